"""GPU: a deformed model keeps its hierarchy (srt_set_acceleration_deform(SRT_DEFORM_REFIT)). After an update with other
vertices the canvas is the array scan's of the deformed mesh, bit for bit; the device's blocks are the host's in-place refit
around the new triangles (srt_bvh_refit_deformed_wide_host); the counters say kept, not built; the cost ratio the device
sums is the host's (srt_bvh_wide_cost_host) within the rounding of a double sum; a tree whose ratio passed rebuild_ratio is
built anew at the next deformation. Frames are 32x18, 4 samples, 3 bounces, from a camera outside and one inside the mesh;
SRT_REFIT_DEVICE unless a test says otherwise."""
import numpy as np
import pytest

import bvh_deform_cases as D
import bvh_refit_cases as K
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
HOST, DEVICE = 0, 1
REBUILD, REFIT = 0, 1
W, H = 32, 18
CAMERAS = [S.default_camera(), R.camera_matrix((0.05, 0.1, 0.0), 0.4, -0.2)]  # outside; inside the blob
MATS = S.sphere_scene()[2]


def scene(*models):
    """a ground plane and the model shapes, all with material 1"""
    shapes = np.zeros(1 + len(models), R.SHAPE)
    shapes[0] = R.plane(0, (0, -1.2, 0), (0, 1, 0))
    for k, m in enumerate(models):
        shapes[1 + k] = m
        shapes[1 + k]["material"] = 1
    return shapes


def handle(T, sky, accel=1, refit=DEVICE, deform=REFIT, ratio=0.0):
    t = T.Tracer(W, H)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    t.set_acceleration_refit(refit)
    t.set_acceleration_deform(deform, ratio)
    return t


def update(t, shapes, tris):
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, MATS)


def frames(t):
    out = []
    for k, cam in enumerate(CAMERAS):
        t.options = R.render_data(W, H, 4, 3, camera_to_world=cam, time=4711 + k)
        t.clear_canvas()
        t.trace()
        out.append(t.read_canvas())
    return out


def same_frames(a, b):
    return len(a) == len(b) and all(bits_equal(x, y) for x, y in zip(a, b))


def scan_frames(T, sky, shapes, tris):
    t = handle(T, sky, accel=0)
    update(t, shapes, tris)
    out = frames(t)
    t.close()
    return out


def tolerance(n_blocks):
    """relative: a double sum of n_blocks non-negative terms in any order is within n_blocks * 2^-53 of the exact one, and so
    is the host's; the quotient of two such sums doubles it"""
    return n_blocks * 2.0 ** -52


_runs = {}


def deformed_run(T, sky, model):
    """update(mesh), clear, update(waved mesh) under SRT_DEFORM_REFIT on the device, once per model: frames, blocks, counters"""
    if model not in _runs:
        t0 = D.base(model)
        t1 = D.wave(t0)
        t = handle(T, sky)
        update(t, scene(D.shape_over(t0)), t0)
        first = (t.acceleration_info(), t.acceleration_deform_info())
        t.clear_canvas()
        update(t, scene(D.shape_over(t1)), t1)
        run = {"t0": t0, "t1": t1, "first": first, "acc": t.acceleration_info(), "deform": t.acceleration_deform_info(),
               "refit": t.acceleration_refit_info(), "blocks": t.read_bvh_blocks(), "frames": frames(t)}
        t.close()
        run["scan"] = scan_frames(T, sky, scene(D.shape_over(t1)), t1)
        _runs[model] = run
    return _runs[model]


@pytest.mark.parametrize("model", D.SIZES)
def test_canvas_of_the_kept_hierarchy_is_the_scans(model, T, sky):
    run = deformed_run(T, sky, model)
    assert same_frames(run["frames"], run["scan"])
    assert len({a.tobytes() for a in run["scan"]}) == 2  # (the two cameras see different things)


@pytest.mark.parametrize("model", D.SIZES)
def test_device_blocks_equal_the_host_deformed_refit(model, T, sky):
    run = deformed_run(T, sky, model)
    t0, t1 = run["t0"], run["t1"]
    want = T.bvh_refit_deformed_wide_host(D.shape_over(t0), t0, D.shape_over(t1), t1)["blocks"]
    inner = want[:, 3] != 0
    got = run["blocks"]
    assert got.shape == want.shape
    assert np.array_equal(got[inner, :12], want[inner, :12])  # (one model: its first block is block 0)
    assert not got[inner, 12:].any()
    assert (int(inner.sum()) > 0) == (len(t0) > 3)


@pytest.mark.parametrize("model", D.SIZES)
def test_counters_and_cost_ratio(model, T, sky):
    run = deformed_run(T, sky, model)
    t0, t1 = run["t0"], run["t1"]
    acc0, deform0 = run["first"]
    assert acc0["models_built"] == 1 and deform0 == {"models_kept": 0, "models_rebuilt": 0, "cost_launches": 0, "worst_ratio": 1.0}
    acc, deform, refit = run["acc"], run["deform"], run["refit"]
    assert (acc["models_built"], acc["models_reused"], acc["models_refitted"]) == (0, 0, 1)
    assert deform["models_kept"] == 1 and deform["models_rebuilt"] == 0 and deform["cost_launches"] >= 1
    assert refit["models"] == 1
    cb, cn = T.bvh_wide_cost_host(D.shape_over(t0), t0, D.shape_over(t1), t1)
    want = cn / cb
    print(f"{model}: ratio device {deform['worst_ratio']!r} host {want!r} blocks {len(run['blocks'])}")
    assert cb > 0.0 and cn > 0.0
    assert abs(deform["worst_ratio"] - want) <= tolerance(len(run["blocks"])) * want


def test_default_mode_rebuilds_and_launches_no_cost_kernel(T, sky):
    t0 = D.base("n200")
    t1 = D.wave(t0)
    t = handle(T, sky, deform=REBUILD)
    update(t, scene(D.shape_over(t0)), t0)
    update(t, scene(D.shape_over(t1)), t1)
    acc, deform, refit = t.acceleration_info(), t.acceleration_deform_info(), t.acceleration_refit_info()
    assert acc["models_built"] == 1 and acc["models_refitted"] == 0
    assert deform == {"models_kept": 0, "models_rebuilt": 0, "cost_launches": 0, "worst_ratio": 0.0}
    assert refit == {"models": 0, "inner_blocks": 0, "launches": 0}
    # a model that only moved: the refit's launches and no other
    moved = D.shape_over(t1, K.MOVES["rotate"])
    update(t, scene(moved), t1)
    want = T.bvh_refit_wide_host(D.shape_over(t1), moved, t1)["blocks"]
    inner = want[:, 3] != 0
    assert t.acceleration_refit_info()["models"] == 1 and t.acceleration_deform_info()["cost_launches"] == 0
    assert np.array_equal(t.read_bvh_blocks()[inner, :12], want[inner, :12])
    got = frames(t)
    for bad in (2, -1):
        with pytest.raises(T.SrtError):
            t.set_acceleration_deform(bad)
    for bad in (1.0, 0.5, -2.0, float("nan"), float("inf")):
        with pytest.raises(T.SrtError):
            t.set_acceleration_deform(REFIT, bad)
    t.close()
    assert same_frames(got, scan_frames(T, sky, scene(moved), t1))


def test_host_refit_mode(T, sky):
    t0 = D.base("n200")
    t1 = D.wave(t0)
    t = handle(T, sky, refit=HOST)
    update(t, scene(D.shape_over(t0)), t0)
    t.clear_canvas()
    update(t, scene(D.shape_over(t1)), t1)
    acc, deform, refit = t.acceleration_info(), t.acceleration_deform_info(), t.acceleration_refit_info()
    got = frames(t)
    t.close()
    assert (acc["models_built"], acc["models_refitted"]) == (0, 1) and deform["models_kept"] == 1
    assert deform["cost_launches"] == 0 and refit["models"] == 0 and deform["worst_ratio"] > 0.0  # (the host's own sum, over its re-folded tree)
    assert same_frames(got, scan_frames(T, sky, scene(D.shape_over(t1)), t1))


def test_deformed_and_moved_in_one_call(T, sky):
    t0 = D.base("n200")
    t1 = D.wave(t0)
    now = D.shape_over(t1, K.MOVES["rotate"])
    t = handle(T, sky)
    update(t, scene(D.shape_over(t0)), t0)
    t.clear_canvas()
    update(t, scene(now), t1)
    acc, deform = t.acceleration_info(), t.acceleration_deform_info()
    blocks, got = t.read_bvh_blocks(), frames(t)
    t.close()
    assert (acc["models_built"], acc["models_refitted"]) == (0, 1) and deform["models_kept"] == 1
    want = T.bvh_refit_deformed_wide_host(D.shape_over(t0), t0, now, t1)["blocks"]
    inner = want[:, 3] != 0
    assert np.array_equal(blocks[inner, :12], want[inner, :12])
    assert same_frames(got, scan_frames(T, sky, scene(now), t1))


def test_two_models_of_different_depth(T, sky):
    """6,050 and 7 triangles stale in one call: the level schedule of both, the cost kernel's blockIdx.y"""
    big, small = D.base("n6k"), D.base("n7")
    xf = R.translate((1.6, 0.3, 0.4))

    def arrays(b, s):
        tris = R.concat(R.TRIANGLE, b, s)
        return scene(D.shape_over(tris, count=len(b)), D.shape_over(tris, xf, first=len(b))), tris

    s0, tris0 = arrays(big, small)
    s1, tris1 = arrays(D.wave(big), D.wave(small))
    t = handle(T, sky)
    update(t, s0, tris0)
    t.clear_canvas()
    update(t, s1, tris1)
    acc, deform, refit = t.acceleration_info(), t.acceleration_deform_info(), t.acceleration_refit_info()
    got = frames(t)
    t.close()
    assert (acc["models_built"], acc["models_refitted"]) == (0, 2) and deform["models_kept"] == 2 and refit["models"] == 2
    ratios, blocks = [], 0
    for shape0, shape1 in zip(s0[1:], s1[1:]):
        cb, cn = T.bvh_wide_cost_host(shape0, tris0, shape1, tris1)
        ratios.append(cn / cb)
        blocks = max(blocks, len(T.bvh_wide_host(shape0, tris0)["blocks"]))
    assert abs(deform["worst_ratio"] - max(ratios)) <= tolerance(blocks) * max(ratios)
    assert same_frames(got, scan_frames(T, sky, s1, tris1))


def test_two_instances_of_one_range(T, sky):
    t0 = D.base("n200")
    t1 = D.wave(t0)
    xf = R.mat_mul(R.translate((1.5, 0.2, -0.5)), R.euler_yxz(0.6, 0.2, -0.3))
    t = handle(T, sky)
    update(t, scene(D.shape_over(t0), D.shape_over(t0, xf)), t0)
    t.clear_canvas()
    s1 = scene(D.shape_over(t1), D.shape_over(t1, xf))
    update(t, s1, t1)
    acc, deform = t.acceleration_info(), t.acceleration_deform_info()
    got = frames(t)
    t.close()
    assert (acc["models_built"], acc["models_reused"], acc["models_refitted"]) == (0, 0, 2) and deform["models_kept"] == 2
    assert same_frames(got, scan_frames(T, sky, s1, t1))


def test_a_nan_vertex_from_the_deformation(T, sky):
    t0 = D.base("n200")
    t1 = D.with_nan(t0)
    t = handle(T, sky)
    update(t, scene(D.shape_over(t0)), t0)
    t.clear_canvas()
    s1 = scene(D.shape_over(t1))
    update(t, s1, t1)
    deform, blocks, got = t.acceleration_deform_info(), t.read_bvh_blocks(), frames(t)
    t.close()
    want = T.bvh_refit_deformed_wide_host(D.shape_over(t0), t0, D.shape_over(t1), t1)["blocks"]
    inner = want[:, 3] != 0
    assert deform["models_kept"] == 1 and np.array_equal(blocks[inner, :12], want[inner, :12])
    cb, cn = T.bvh_wide_cost_host(D.shape_over(t0), t0, D.shape_over(t1), t1)
    assert abs(deform["worst_ratio"] - cn / cb) <= tolerance(len(want)) * (cn / cb)
    assert same_frames(got, scan_frames(T, sky, s1, t1))


@pytest.mark.parametrize("model", ["n200", "n6k"])
def test_rebuild_policy(model, T, sky):
    """rebuild_ratio just below the scramble's host ratio, far above the wave's (tests/test_bvh_deform_host.py checks the
    factor of two between them): waves keep the tree, the update AFTER a scramble builds a new one."""
    wave_ratio, scramble_ratio = D.ratios(model)
    assert scramble_ratio >= 2.0 * wave_ratio
    bound = 0.98 * scramble_ratio
    t0 = D.base(model)
    n_blocks = len(T.bvh_wide_host(D.shape_over(t0), t0)["blocks"])
    t = handle(T, sky, ratio=bound)
    scan = handle(T, sky, accel=0)
    steps = [("base", t0), ("wave", D.wave(t0)), ("scramble", D.scramble(t0)), ("wave2", D.wave(t0, step=2)), ("wave3", D.wave(t0, step=3))]
    seen = {}
    for name, tris in steps:
        shapes = scene(D.shape_over(tris))
        update(t, shapes, tris)
        update(scan, shapes, tris)
        seen[name] = (t.acceleration_info(), t.acceleration_deform_info())
        print(name, seen[name][1])
        assert same_frames(frames(t), frames(scan)), name
    t.close()
    scan.close()
    for name in ("wave", "scramble", "wave3"):
        acc, deform = seen[name]
        assert deform["models_kept"] == 1 and deform["models_rebuilt"] == 0 and acc["models_built"] == 0, name
    assert abs(seen["wave"][1]["worst_ratio"] - wave_ratio) <= tolerance(n_blocks) * wave_ratio
    assert abs(seen["scramble"][1]["worst_ratio"] - scramble_ratio) <= tolerance(n_blocks) * scramble_ratio
    acc, deform = seen["wave2"]
    assert deform["models_rebuilt"] == 1 and deform["models_kept"] == 0 and acc["models_built"] == 1
    assert abs(deform["worst_ratio"] - 1.0) <= tolerance(n_blocks)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_group_of_virtual_devices(devices, T, sky):
    t0 = D.base("n200")
    t1 = D.wave(t0)
    canv = []
    for group in (False, True):
        t = T.TracerGroup(W, H, n_devices=len(devices), devices=devices, rows_per_block=2) if group else T.Tracer(W, H)
        t.set_skybox(sky)
        t.set_acceleration(1)
        t.set_acceleration_refit(DEVICE)
        t.set_acceleration_deform(REFIT)
        t.options = R.render_data(W, H, 4, 3, camera_to_world=S.default_camera(), time=99)
        update(t, scene(D.shape_over(t0)), t0)
        update(t, scene(D.shape_over(t1)), t1)
        infos = [t.member_deform_info(i) for i in range(len(devices))] if group else [t.acceleration_deform_info()]
        t.clear_canvas()
        t.render(1)
        canv.append(t.read_canvas())
        t.close()
        assert all(i["models_kept"] == 1 and i["cost_launches"] >= 1 for i in infos), infos
        ratios = [i["worst_ratio"] for i in infos]
        assert min(ratios) > 0.0 and max(ratios) - min(ratios) <= tolerance(200) * max(ratios)  # (under 200 blocks; each member sums for itself)
    assert bits_equal(canv[1], canv[0])


def test_twenty_wave_steps_without_a_rebuild(T, sky):
    """a slip in the stale mark or in the entry's tris / tri_hash shows as a wrong canvas or as a build"""
    t0 = D.base("n200")
    t = handle(T, sky)
    scan = handle(T, sky, accel=0)
    update(t, scene(D.shape_over(t0)), t0)
    for step in range(1, 21):
        tris = D.wave(t0, step=step, amplitude=0.05)
        shapes = scene(D.shape_over(tris))
        update(t, shapes, tris)
        acc, deform = t.acceleration_info(), t.acceleration_deform_info()
        assert acc["models_built"] == 0 and acc["models_refitted"] == 1 and deform["models_kept"] == 1, step
        if step in (1, 10, 20):
            update(scan, shapes, tris)
            assert same_frames(frames(t), frames(scan)), step
    t.close()
    scan.close()
