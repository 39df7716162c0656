"""GPU: SRT_BUILD_DEVICE under SRT_BUILD_ORDER_MEDIAN (srt_set_acceleration_build_order): the balanced topology over the median-split
order. The canvas is the array scan's, bit for bit; the device's blocks are the host statement's (srt_bvh_median_wide_host) and
its leaves hold the triangles of the host's order (srt_bvh_median_order_host); the launches are those the count asks for
(tests/bvh_median_cases.py launches: stated from SRT_BUILD_LOCAL = 1,024 and the count); afterwards the model is re-used, moved
and deformed like any other. Frames are 32x18, 4 samples, 3 bounces, from a camera outside and one inside the mesh.
The prefixes of n6k: no split (1, 3), the first split (4), ragged halves (5, 7, 8), a wave and a round of the local launch (64,
65, 257), the local launch alone against one global level (1,023, 1,024, 1,025), two ranges (2,048, 2,049), two global levels
with ranges of unequal size (4,099); n6k itself takes three, ragged everywhere."""
import sys

import numpy as np
import pytest

import bvh_build_cases as B
import bvh_deform_cases as D
import bvh_median_cases as M
import bvh_refit_cases as K
import test_gpu_bvh_deform as G
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S
from test_gpu_bvh_refit import levels_of

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(10000)
HOST, DEVICE = 0, 1
REBUILD, REFIT = 0, 1
MORTON, MEDIAN = 0, 1
NO_BUILD = {"models": 0, "records": 0, "launches": 0}
MORTON_LAUNCHES = 1 + 1 + 4 * 3  # extents, codes, and per pass of the sort a histogram, a scan and a scatter


def handle(T, sky, accel=1, refit=HOST, deform=REBUILD, build=DEVICE, min_triangles=0, order=MEDIAN):
    t = G.handle(T, sky, accel=accel, refit=refit, deform=deform)
    t.set_acceleration_build(build, min_triangles)
    t.set_acceleration_build_order(order)
    return t


def check_blocks(T, blocks, model, tris, first=0, statement="median"):
    """the model's blocks from block `first` on: the inner ones are the host statement's, the leaves hold its order. Returns the
    model's block count."""
    want = getattr(T, f"bvh_{statement}_wide_host")(model, tris)
    order = getattr(T, f"bvh_{statement}_order_host")(model, tris)
    wb = want["blocks"].copy()
    inner = wb[:, 3] != 0
    wb[inner, 11] += first  # absolute indices
    mine = blocks[first:first + len(wb)]
    assert mine.shape == wb.shape
    assert np.array_equal(mine[inner, :12], wb[inner, :12])
    assert not mine[inner, 12:].any()
    dest = want["dest"]
    assert np.array_equal(mine[dest >> 2, 28 + (dest & 3)], order)  # every record's triangle, as the pre-pass found it in `order`
    return len(wb)


_runs = {}


def built_run(T, sky, model, variant):
    """update(mesh) under the median order, once per mesh: counters, blocks, frames, and the scan's frames"""
    if (model, variant) not in _runs:
        tris = B.mesh(model, variant)
        shapes = G.scene(D.shape_over(tris))
        t = handle(T, sky)
        G.update(t, shapes, tris)
        run = {"tris": tris, "build": t.acceleration_build_info(), "acc": t.acceleration_info(), "refit": t.acceleration_refit_info(),
               "blocks": t.read_bvh_blocks(), "frames": G.frames(t)}
        t.close()
        run["scan"] = G.scan_frames(T, sky, shapes, tris)
        _runs[(model, variant)] = run
    return _runs[(model, variant)]


@pytest.mark.parametrize("model,variant", M.CASES)
def test_canvas_is_the_scans(model, variant, T, sky):
    run = built_run(T, sky, model, variant)
    assert G.same_frames(run["frames"], run["scan"])
    assert len({a.tobytes() for a in run["scan"]}) == 2  # (the two cameras see different things)


@pytest.mark.parametrize("model,variant", M.CASES)
def test_device_blocks_are_the_host_statements(model, variant, T, sky):
    run = built_run(T, sky, model, variant)
    tris = run["tris"]
    n = len(tris)
    n_blocks = check_blocks(T, run["blocks"], D.shape_over(tris), tris)
    assert n_blocks == len(run["blocks"])
    assert run["build"] == {"models": 1, "records": n, "launches": M.launches(n)}
    assert (run["acc"]["models_built"], run["acc"]["models_reused"], run["acc"]["models_refitted"]) == (1, 0, 0)
    want = T.bvh_median_wide_host(D.shape_over(tris), tris)["blocks"]
    assert run["refit"] == {"models": 1, "inner_blocks": int((want[:, 3] != 0).sum()), "launches": 2 + levels_of(want)}
    if model == "n6k" and variant == "base":
        assert M.launches(n) == 3 * (2 + 9) + 1
        order = T.bvh_median_order_host(D.shape_over(tris), tris)
        assert not np.array_equal(order, np.arange(n)) and not np.array_equal(order, T.bvh_morton_order_host(D.shape_over(tris), tris))


def test_three_models_of_different_depth(T, sky):
    """n6k (three global levels), a 200-triangle model (the local launch alone: its workgroups return whole from every global
    launch) and a 7-triangle model below min_triangles that the host builds, in one update"""
    big, mid, small = D.base("n6k"), D.base("n200"), D.base("n7")
    tris = R.concat(R.TRIANGLE, big, mid, small)
    models = [D.shape_over(tris, count=len(big)), D.shape_over(tris, R.mat_mul(R.translate((2.2, 0.2, -0.5)), R.euler_yxz(0.6, 0.2, -0.3)), first=len(big), count=200),
              D.shape_over(tris, R.translate((-2.0, 0.3, 0.4)), first=len(big) + 200)]
    shapes = G.scene(*models)
    t = handle(T, sky, min_triangles=100)
    G.update(t, shapes, tris)
    build, acc, refit = t.acceleration_build_info(), t.acceleration_info(), t.acceleration_refit_info()
    blocks, got = t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert build == {"models": 2, "records": len(big) + 200, "launches": M.launches(len(big))}  # (the level loop is the deepest model's)
    assert (acc["models_built"], acc["models_reused"], acc["models_refitted"]) == (3, 0, 0) and refit["models"] == 2
    first = 0
    for m in models[:2]:
        first += check_blocks(T, blocks, m, tris, first)
    sah = T.bvh_wide_host(models[2], tris)["blocks"]
    inner = sah[:, 3] != 0
    sah[inner, 11] += first
    assert len(blocks) == first + len(sah) and np.array_equal(blocks[first:][inner, :12], sah[inner, :12])
    assert G.same_frames(got, G.scan_frames(T, sky, shapes, tris))


@pytest.mark.parametrize("refit", [HOST, DEVICE])
def test_afterlife_moved(refit, T, sky):
    """after a median build: a move -- by the host, which needs the order back, and by the device, which keeps it"""
    tris = D.base("n6k")
    built, moved = D.shape_over(tris), D.shape_over(tris, K.MOVES["rotate"])
    t = handle(T, sky, refit=refit)
    G.update(t, G.scene(built), tris)
    assert t.acceleration_build_info() == {"models": 1, "records": len(tris), "launches": M.launches(len(tris))}
    G.update(t, G.scene(moved), tris)
    acc, refit_info, build = t.acceleration_info(), t.acceleration_refit_info(), t.acceleration_build_info()
    blocks, got = t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert build == NO_BUILD and (acc["models_built"], acc["models_reused"], acc["models_refitted"]) == (0, 0, 1)
    assert refit_info["models"] == (1 if refit == DEVICE else 0)
    if refit == DEVICE:  # the in-place refit of the median tree around the moved model: the median statement of the moved model's
        # topology and order are the built model's only if the order is -- compare the leaves through the built model's order
        want = T.bvh_median_wide_host(built, tris)
        order = T.bvh_median_order_host(built, tris)
        assert np.array_equal(blocks[want["dest"] >> 2, 28 + (want["dest"] & 3)], order)
    assert G.same_frames(got, G.scan_frames(T, sky, G.scene(moved), tris))


def test_afterlife_deformed(T, sky):
    """under SRT_DEFORM_REFIT the build is measured (ratio 1), and the next deformation keeps the tree and the order"""
    t0 = D.base("n6k")
    t1 = D.wave(t0)
    want = T.bvh_median_wide_host(D.shape_over(t0), t0)
    n_blocks = len(want["blocks"])
    t = handle(T, sky, refit=DEVICE, deform=REFIT)
    G.update(t, G.scene(D.shape_over(t0)), t0)
    build, deform = t.acceleration_build_info(), t.acceleration_deform_info()
    assert build["models"] == 1 and build["launches"] == M.launches(len(t0)) and deform["models_kept"] == 0 and deform["cost_launches"] >= 1
    print(f"ratio after the build {deform['worst_ratio']!r}")
    assert abs(deform["worst_ratio"] - 1.0) <= G.tolerance(n_blocks)
    G.update(t, G.scene(D.shape_over(t1)), t1)
    build, deform, acc = t.acceleration_build_info(), t.acceleration_deform_info(), t.acceleration_info()
    blocks, got = t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert build == NO_BUILD and deform["models_kept"] == 1 and deform["models_rebuilt"] == 0
    assert (acc["models_built"], acc["models_refitted"]) == (0, 1)
    assert np.array_equal(blocks[want["dest"] >> 2, 28 + (want["dest"] & 3)], T.bvh_median_order_host(D.shape_over(t0), t0))
    assert deform["worst_ratio"] > 0.0
    assert G.same_frames(got, G.scan_frames(T, sky, G.scene(D.shape_over(t1)), t1))


def test_rebuild_on_cost_goes_to_the_median_launches(T, sky):
    """a tree whose ratio passed rebuild_ratio is built anew -- on the device, in the order in force"""
    t0 = B.mesh(f"p{M.LOCAL + 1}")
    t = handle(T, sky, refit=DEVICE, deform=REFIT)
    t.set_acceleration_deform(REFIT, 1.5)
    G.update(t, G.scene(D.shape_over(t0)), t0)
    scr = D.scramble(t0)
    G.update(t, G.scene(D.shape_over(scr)), scr)
    assert t.acceleration_deform_info()["worst_ratio"] > 1.5 and t.acceleration_build_info() == NO_BUILD
    t2 = D.wave(t0, step=2)
    shapes = G.scene(D.shape_over(t2))
    G.update(t, shapes, t2)
    deform, build = t.acceleration_deform_info(), t.acceleration_build_info()
    blocks, got = t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert deform["models_rebuilt"] == 1 and build == {"models": 1, "records": len(t2), "launches": M.launches(len(t2))}
    assert M.launches(len(t2)) == 2 + 9 + 1 and abs(deform["worst_ratio"] - 1.0) <= G.tolerance(len(blocks))
    check_blocks(T, blocks, D.shape_over(t2), t2)
    assert G.same_frames(got, G.scan_frames(T, sky, shapes, t2))


def test_back_to_the_morton_order(T, sky):
    """MEDIAN, then MORTON on the same handle and another mesh: the Morton statement's blocks from its 14 launches"""
    t0, t1 = D.base("n6k"), B.mesh(f"p{2 * M.LOCAL + 1}")
    t = handle(T, sky)
    G.update(t, G.scene(D.shape_over(t0)), t0)
    assert t.acceleration_build_info()["launches"] == M.launches(len(t0))
    t.set_acceleration_build_order(MORTON)
    shapes = G.scene(D.shape_over(t1))
    G.update(t, shapes, t1)
    build, blocks, got = t.acceleration_build_info(), t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert build == {"models": 1, "records": len(t1), "launches": MORTON_LAUNCHES}
    check_blocks(T, blocks, D.shape_over(t1), t1, statement="morton")
    assert G.same_frames(got, G.scan_frames(T, sky, shapes, t1))


def test_setter(T, sky):
    tris = D.base("n200")
    shapes = G.scene(D.shape_over(tris))
    t = handle(T, sky, build=HOST)  # accepted and without effect under SRT_BUILD_HOST
    for bad in (2, -1):
        with pytest.raises(T.SrtError):
            t.set_acceleration_build_order(bad)
    G.update(t, shapes, tris)
    assert t.acceleration_build_info() == NO_BUILD and t.acceleration_info()["models_built"] == 1
    sah = T.bvh_wide_host(D.shape_over(tris), tris)["blocks"]
    inner = sah[:, 3] != 0
    assert np.array_equal(t.read_bvh_blocks()[inner, :12], sah[inner, :12])
    t.set_acceleration(0)  # ... and under the array scan
    G.update(t, shapes, tris)
    assert t.acceleration_build_info() == NO_BUILD
    t.set_acceleration(1)
    t.set_acceleration_build(DEVICE)  # the order set earlier is in force; the timer spans the launches
    t.set_kernel_timers(True)
    t1 = D.wave(tris)
    G.update(t, G.scene(D.shape_over(t1)), t1)
    assert t.acceleration_build_info() == {"models": 1, "records": 200, "launches": 1} and t.last_build_kernel_ms() > 0.0
    check_blocks(T, t.read_bvh_blocks(), D.shape_over(t1), t1)
    t.close()


def test_group_of_virtual_devices(T, sky):
    tris = D.base("n6k")
    shapes = G.scene(D.shape_over(tris))
    canv = []
    for group in (False, True):
        t = T.TracerGroup(G.W, G.H, n_devices=2, devices=[0, 0], rows_per_block=2) if group else T.Tracer(G.W, G.H)
        t.set_skybox(sky)
        t.set_acceleration(1)
        t.set_acceleration_build(DEVICE)
        t.set_acceleration_build_order(MEDIAN)
        t.options = R.render_data(G.W, G.H, 4, 3, camera_to_world=S.default_camera(), time=99)
        G.update(t, shapes, tris)
        infos = [t.member_build_info(i) for i in range(2)] if group else [t.acceleration_build_info()]
        G.update(t, shapes, tris)  # (the first member's read-back serves the host's refit of the group's one cache)
        t.clear_canvas()
        t.render(1)
        canv.append(t.read_canvas())
        t.close()
        assert all(i == {"models": 1, "records": len(tris), "launches": M.launches(len(tris))} for i in infos), infos
    assert bits_equal(canv[1], canv[0])
