"""GPU: a model's hierarchy built on the device (srt_set_acceleration_build(SRT_BUILD_DEVICE)): the Morton sort under the balanced
topology. The canvas is the array scan's, bit for bit; the device's blocks are the host statement's (srt_bvh_morton_wide_host)
and its leaves hold the triangles of the host's Morton order (srt_bvh_morton_order_host) -- the two checks that catch a wrong
sort; the counters say who built what; afterwards the model is re-used, moved and deformed like any other. Frames are 32x18,
4 samples, 3 bounces, from a camera outside and one inside the mesh (tests/test_gpu_bvh_deform.py's).
The sort's tile is 1,024 records (csrc/device_types.h SRT_BUILD_TILE), four rounds of 256: the prefixes of n6k cross a wave
(64, 65), a round (256, 257), one tile (1,024, 1,025) and two (2,048, 2,049); n6k itself has a ragged sixth tile."""
import sys

import numpy as np
import pytest

import bvh_build_cases as B
import bvh_deform_cases as D
import bvh_refit_cases as K
import test_gpu_bvh_deform as G
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S
from test_bvh_morton_host import line_mesh
from test_gpu_bvh_refit import levels_of

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(10000)
HOST, DEVICE = 0, 1
REBUILD, REFIT = 0, 1
assert B.TILE == 1024
CASES = [(m, v) for v in B.VARIANTS for m in D.SIZES] + [(f"p{n}", "base") for n in B.SORT_SIZES]
NO_BUILD = {"models": 0, "records": 0, "launches": 0}
SORT_LAUNCHES = 1 + 1 + 4 * 3  # extents, codes, and per pass of the sort a histogram, a scan and a scatter


def handle(T, sky, accel=1, refit=HOST, deform=REBUILD, build=DEVICE, min_triangles=0):
    t = G.handle(T, sky, accel=accel, refit=refit, deform=deform)
    if build is not None:
        t.set_acceleration_build(build, min_triangles)
    return t


_runs = {}


def built_run(T, sky, model, variant):
    """update(mesh) under SRT_BUILD_DEVICE, once per mesh: counters, blocks, frames, and the scan's frames"""
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


@pytest.mark.parametrize("model,variant", CASES)
def test_canvas_is_the_scans(model, variant, T, sky):
    run = built_run(T, sky, model, variant)
    assert G.same_frames(run["frames"], run["scan"])
    assert len({a.tobytes() for a in run["scan"]}) == 2  # (the two cameras see different things)


@pytest.mark.parametrize("model,variant", CASES)
def test_device_blocks_are_the_host_statements(model, variant, T, sky):
    run = built_run(T, sky, model, variant)
    tris = run["tris"]
    n = len(tris)
    want = T.bvh_morton_wide_host(D.shape_over(tris), tris)
    order = T.bvh_morton_order_host(D.shape_over(tris), tris)
    inner = want["blocks"][:, 3] != 0
    got = run["blocks"]
    assert got.shape == want["blocks"].shape
    assert np.array_equal(got[inner, :12], want["blocks"][inner, :12])  # (one model: its first block is block 0)
    assert not got[inner, 12:].any()
    dest = want["dest"]
    assert np.array_equal(got[dest >> 2, 28 + (dest & 3)], order)  # every record's triangle, as the pre-pass found it in `order`
    assert run["build"] == {"models": 1, "records": n, "launches": SORT_LAUNCHES}
    assert (run["acc"]["models_built"], run["acc"]["models_reused"], run["acc"]["models_refitted"]) == (1, 0, 0)
    assert run["refit"] == {"models": 1, "inner_blocks": int(inner.sum()), "launches": 2 + levels_of(want["blocks"])}
    if model == "n6k" and variant == "base":
        assert not np.array_equal(order, np.arange(n))


def test_scene_mix(T, sky):
    """two instances of one 200-triangle range under different transforms and a 7-triangle model, min_triangles between: the
    instances are built on the device (blockIdx.y, two tables), the small one by the host's SAH"""
    big, small = D.base("n200"), D.base("n7")
    tris = R.concat(R.TRIANGLE, big, small)
    xf = R.mat_mul(R.translate((1.5, 0.2, -0.5)), R.euler_yxz(0.6, 0.2, -0.3))
    models = [D.shape_over(tris, count=200), D.shape_over(tris, xf, count=200), D.shape_over(tris, R.translate((-1.4, 0.3, 0.4)), first=200)]
    shapes = G.scene(*models)
    t = handle(T, sky, min_triangles=100)
    G.update(t, shapes, tris)
    build, acc, refit = t.acceleration_build_info(), t.acceleration_info(), t.acceleration_refit_info()
    blocks, got = t.read_bvh_blocks(), G.frames(t)
    t.close()
    assert build == {"models": 2, "records": 400, "launches": SORT_LAUNCHES}
    assert (acc["models_built"], acc["models_reused"], acc["models_refitted"]) == (3, 0, 0) and refit["models"] == 2
    first = 0
    for m in models[:2]:
        want = T.bvh_morton_wide_host(m, tris)
        wb = want["blocks"].copy()
        inner = wb[:, 3] != 0
        wb[inner, 11] += first  # absolute indices
        mine = blocks[first:first + len(wb)]
        assert np.array_equal(mine[inner, :12], wb[inner, :12])
        assert np.array_equal(mine[want["dest"] >> 2, 28 + (want["dest"] & 3)], T.bvh_morton_order_host(m, tris))
        first += len(wb)
    sah = T.bvh_wide_host(models[2], tris)["blocks"]
    inner = sah[:, 3] != 0
    sah[inner, 11] += first
    assert len(blocks) == first + len(sah) and np.array_equal(blocks[first:][inner, :12], sah[inner, :12])
    assert G.same_frames(got, G.scan_frames(T, sky, shapes, tris))


@pytest.mark.parametrize("refit", [HOST, DEVICE])
def test_afterlife_moved_and_reused(refit, T, sky):
    """after a device build: the same bytes again, then a move -- by the host, which needs the sorted order back, and by the
    device, which keeps it -- and the same bytes once more"""
    tris = D.base("n6k")
    built, moved = D.shape_over(tris), D.shape_over(tris, K.MOVES["rotate"])
    t = handle(T, sky, refit=refit)
    G.update(t, G.scene(built), tris)
    assert t.acceleration_build_info()["models"] == 1
    scans = {}
    for step, shape in (("same", built), ("moved", moved), ("same again", moved)):
        G.update(t, G.scene(shape), tris)
        acc, refit_info = t.acceleration_info(), t.acceleration_refit_info()
        assert t.acceleration_build_info() == NO_BUILD and acc["models_built"] == 0, step
        if refit == DEVICE:  # re-used as it is (its boxes are refitted with every upload), or refitted after the move
            assert (acc["models_reused"], acc["models_refitted"]) == ((0, 1) if step == "moved" else (1, 0)), step
            assert refit_info["models"] == 1, step
        else:  # the host makes the boxes it never had, once: after that the entry is like any host-built one
            assert (acc["models_reused"], acc["models_refitted"]) == ((1, 0) if step == "same again" else (0, 1)), step
            assert refit_info["models"] == 0, step
        key = shape["transform"].tobytes()
        if key not in scans:
            scans[key] = G.scan_frames(T, sky, G.scene(shape), tris)
        assert G.same_frames(G.frames(t), scans[key]), step
    t.close()


def test_afterlife_deformed(T, sky):
    """under SRT_DEFORM_REFIT the build is measured: its cost is the tree's cost as built (ratio 1), and the next deformation
    keeps the tree -- with the ratio of the host statement's costs (the refitted tree's from earlier calls, as
    tests/test_bvh_morton_host.py builds its expectation)"""
    t0 = D.base("n6k")
    t1 = D.wave(t0)
    n = len(t0)
    want = T.bvh_morton_wide_host(D.shape_over(t0), t0)
    n_blocks = len(want["blocks"])
    t = handle(T, sky, refit=DEVICE, deform=REFIT)
    G.update(t, G.scene(D.shape_over(t0)), t0)
    build, deform = t.acceleration_build_info(), t.acceleration_deform_info()
    assert build["models"] == 1 and deform["models_kept"] == 0 and deform["cost_launches"] >= 1
    print(f"ratio after the build {deform['worst_ratio']!r}")
    assert abs(deform["worst_ratio"] - 1.0) <= G.tolerance(n_blocks)
    G.update(t, G.scene(D.shape_over(t1)), t1)
    build, deform, acc = t.acceleration_build_info(), t.acceleration_deform_info(), t.acceleration_info()
    got = G.frames(t)
    t.close()
    assert build == NO_BUILD and deform["models_kept"] == 1 and deform["models_rebuilt"] == 0
    assert (acc["models_built"], acc["models_refitted"]) == (0, 1)
    line = line_mesh(n)
    ob = T.bvh_wide_order_host(D.shape_over(line), line, force_balanced=True)
    now = t1.copy()
    now[ob] = t1[T.bvh_morton_order_host(D.shape_over(t0), t0)]
    _, cost_now = T.bvh_wide_cost_host(D.shape_over(line), line, D.shape_over(now), now, force_balanced=True)
    ratio = cost_now / want["cost"]
    print(f"ratio after the wave: device {deform['worst_ratio']!r} host {ratio!r}")
    # both of the device's sums are within n_blocks * 2^-53 of the exact ones, and both of the host's: twice the tolerance of a
    # device quotient over a host denominator
    assert want["cost"] > 0.0 and abs(deform["worst_ratio"] - ratio) <= 2.0 * G.tolerance(n_blocks) * ratio
    assert G.same_frames(got, G.scan_frames(T, sky, G.scene(D.shape_over(t1)), t1))


def test_rebuild_on_cost_goes_to_the_device(T, sky):
    """a tree whose ratio passed rebuild_ratio is built anew -- by the sort"""
    t0 = D.base("n200")
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
    assert deform["models_rebuilt"] == 1 and build["models"] == 1 and abs(deform["worst_ratio"] - 1.0) <= G.tolerance(len(blocks))
    want = T.bvh_morton_wide_host(D.shape_over(t2), t2)["blocks"]
    inner = want[:, 3] != 0
    assert np.array_equal(blocks[inner, :12], want[inner, :12])
    assert G.same_frames(got, G.scan_frames(T, sky, shapes, t2))


def test_group_of_virtual_devices(T, sky):
    tris = D.base("n6k")
    shapes = G.scene(D.shape_over(tris))
    canv = []
    for group in (False, True):
        t = T.TracerGroup(G.W, G.H, n_devices=2, devices=[0, 0], rows_per_block=2) if group else T.Tracer(G.W, G.H)
        t.set_skybox(sky)
        t.set_acceleration(1)
        t.set_acceleration_build(DEVICE)
        t.options = R.render_data(G.W, G.H, 4, 3, camera_to_world=S.default_camera(), time=99)
        G.update(t, shapes, tris)
        infos = [t.member_build_info(i) for i in range(2)] if group else [t.acceleration_build_info()]
        G.update(t, shapes, tris)  # (the first member's read-back serves the host's refit of the group's one cache)
        t.clear_canvas()
        t.render(1)
        canv.append(t.read_canvas())
        t.close()
        assert all(i == {"models": 1, "records": len(tris), "launches": SORT_LAUNCHES} for i in infos), infos
    assert bits_equal(canv[1], canv[0])


def test_default_is_the_host_build(T, sky):
    """the switch never touched: nothing is built on the device, and a move under SRT_REFIT_DEVICE reads what it read before"""
    built, moved, tris = K.shapes_of("n200", "rotate")
    t = handle(T, sky, refit=DEVICE, build=None)
    G.update(t, G.scene(built), tris)
    assert t.acceleration_build_info() == NO_BUILD and t.acceleration_refit_info() == {"models": 0, "inner_blocks": 0, "launches": 0}
    assert t.acceleration_info()["models_built"] == 1
    G.update(t, G.scene(moved), tris)
    want = T.bvh_refit_wide_host(built, moved, tris)["blocks"]
    inner = want[:, 3] != 0
    assert t.acceleration_build_info() == NO_BUILD
    assert t.acceleration_refit_info() == {"models": 1, "inner_blocks": int(inner.sum()), "launches": 2 + levels_of(want)}
    assert np.array_equal(t.read_bvh_blocks()[inner, :12], want[inner, :12])
    t.set_kernel_timers(True)
    G.update(t, G.scene(built), tris)
    assert t.last_build_kernel_ms() == 0.0
    t.close()


def test_setter_and_timer(T, sky):
    tris = D.base("n200")
    shapes = G.scene(D.shape_over(tris))
    t = handle(T, sky, accel=0)  # accepted and without effect under the array scan
    for bad in (2, -1):
        with pytest.raises(T.SrtError):
            t.set_acceleration_build(bad)
    G.update(t, shapes, tris)
    assert t.acceleration_build_info() == NO_BUILD
    scan = G.frames(t)
    t.set_acceleration(1)
    t.set_kernel_timers(True)
    G.update(t, shapes, tris)
    assert t.acceleration_build_info()["models"] == 1 and t.last_build_kernel_ms() > 0.0
    assert G.same_frames(G.frames(t), scan)
    t.set_acceleration_build(DEVICE, 201)  # one triangle too many for the device
    t1 = D.wave(tris)
    G.update(t, G.scene(D.shape_over(t1)), t1)
    assert t.acceleration_build_info() == NO_BUILD and t.acceleration_info()["models_built"] == 1 and t.last_build_kernel_ms() == 0.0
    t.close()
