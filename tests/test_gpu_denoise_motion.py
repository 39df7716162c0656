"""GPU: object motion for the denoiser's temporal stage (srt_set_denoise_object_motion) -- the shape indices of the feature
pass against the oracle, nothing moved = object motion off bit for bit, moved shapes against tests/temporal_ref.py, the rules
that keep or drop the history, the error codes, and quality against the spatial filter while a shape is dragged."""
import json

import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import temporal_ref as TR
from conftest import bits_equal
from gpu_harness import SCENES, T, cam_at, guide_scene, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import scenes as S

pytestmark = pytest.mark.gpu


def history(t):
    hist = t.read_denoise_history()
    hist["ids"] = t.read_denoise_shape_ids()[1]
    return hist


# ---- 4. shape indices -------------------------------------------------------------------------------------------------------
def oracle_ids(oracle, t, shapes, tris, mats, w, h):
    own = np.frombuffer(bytearray(shapes.tobytes()), shapes.dtype)
    has = own["material"] >= 0
    own["material"] = np.where(has, np.arange(len(own)), -1)  # a material per shape: the hit's material names the shape
    mats_own = np.resize(mats, max(len(own), 1))
    hit = oracle.primary_hits(t.options, t.scene_data, own, tris, mats_own, np.arange(w * h), np.zeros(w * h, np.int32))
    return np.where(hit["material"] >= 0, hit["material"], M.NO_SHAPE).astype(np.uint32).reshape(h, w)


def run_ids(T, sky, oracle, name, w, h, accel, dispatches=((3, 4096), (2, 31337))):
    shapes, tris, mats, cam = guide_scene(name)
    t = make(T, sky, (shapes, tris, mats), w, h, spp=1, accel=accel, denoise=dict(iterations=0), temporal={}, motion=True, cam=cam)
    got = []
    for i, (ns, tm) in enumerate(dispatches):
        t.options["num_samples"] = ns
        t.options["time"] = tm
        t.render(i + 1)
        ids = t.read_denoise_shape_ids()[0]
        assert np.array_equal(ids, oracle_ids(oracle, t, shapes, tris, mats, w, h)), (name, accel, i)  # the latest dispatch's
        got.append(ids)
    t.close()
    return got


@pytest.mark.parametrize("name,accel", SCENES)
def test_shape_ids_equal_oracle(T, sky, oracle, name, accel):
    a, b = run_ids(T, sky, oracle, name, 37, 29, accel)
    if name == "empty":
        assert np.all(a == M.NO_SHAPE)
    else:
        assert (a != M.NO_SHAPE).any()
    if name == "mixed":  # another jitter: the second dispatch's buffer is not the first's
        assert not np.array_equal(a, b)
    if name == "no_material":
        assert not np.isin(a, [1, 4]).any()


@pytest.mark.parametrize("name", ["mixed", "mesh_smooth", "mesh_flat", "no_material"])
def test_shape_ids_scan_and_bvh_agree(T, sky, oracle, name):
    for a, b in zip(run_ids(T, sky, oracle, name, 37, 29, 0), run_ids(T, sky, oracle, name, 37, 29, 1)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h", [(1, 33), (33, 1)])
def test_shape_ids_ragged_frames(T, sky, oracle, w, h):
    run_ids(T, sky, oracle, "mixed", w, h, 1)


def test_shape_ids_full_hd(T, sky, oracle):
    run_ids(T, sky, oracle, "spheres", 1920, 1080, 0, dispatches=((1, 4096), (1, 99)))


# ---- 5. nothing moved: object motion on = off, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "move"])
def test_nothing_moved_equals_motion_off(T, sky, kind):
    w, h = 96, 64
    scn = S.mixed_test_scene()
    off = make(T, sky, scn, w, h, accel=1, denoise={}, temporal={})
    on = make(T, sky, scn, w, h, accel=1, denoise={}, temporal={}, motion=True)
    for k in range(5):
        outs = []
        for t in (off, on):
            t.clear_canvas()
            t.update_scene(*scn)
            t.options["camera_to_world"] = cam_at(k, kind)
            t.options["time"] = 300 + k
            outs.append(t.render(1).copy())
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(off.read_denoised(), on.read_denoised()), k
        assert bits_equal(off.read_denoise_inputs()["normal_depth"], on.read_denoise_inputs()["normal_depth"]), k
        if k:
            assert not on.read_denoise_motion()["any_moved"]
    for t in (off, on):
        t.clear_canvas()
    a, b = off.read_denoise_history(), on.read_denoise_history()
    assert a["valid"] and b["valid"] and a["count"].max() > 2
    for key in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(a[key], b[key]), key
    off.close()
    on.close()


# ---- 6. something moved, against numpy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.MOVES, ids=[m[0] for m in M.MOVES])
def test_moved_shapes_match_numpy(T, sky, case):
    """tests/test_motion_reference.py asserts on the CPU that these moves flag at most 1 % of a frame's pixels"""
    name, scn_name, accel, cam_kind, steps = case
    w, h = M.SIZE
    shapes, tris, mats = scene(scn_name)
    tp = dict(history_limit=64, normal_threshold=0.9, depth_threshold=0.05)
    t = make(T, sky, (shapes, tris, mats), w, h, accel=accel, denoise=dict(iterations=0), temporal=tp, motion=True, cam=cam_at(0, cam_kind))
    t.render(1)
    moved_idx = [s[0] for s in steps]
    for k in range(1, M.FRAMES):
        t.clear_canvas()
        hist = history(t)
        assert hist["valid"]
        now = M.move_shapes(shapes, tris, steps, k)
        t.update_scene(now, tris, mats)
        assert t.read_denoise_history()["valid"], k  # the move kept the history
        table = t.read_denoise_motion()
        want_table = M.scene_table((M.move_shapes(shapes, tris, steps, k - 1), tris, mats, t.scene_data), (now, tris, mats, t.scene_data))
        assert table["any_moved"] and table["state"].tolist() == want_table["state"].tolist()
        assert np.array_equal(table["A"], want_table["A"]) or np.abs(table["A"] - want_table["A"]).max() < 1e-6
        t.options["camera_to_world"] = cam_at(k, cam_kind)
        t.options["time"] = 2000 + k
        argb = t.render(1).copy().reshape(h, w, 4)
        inp = t.read_denoise_inputs()
        ids = t.read_denoise_shape_ids()[0]
        want = TR.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, ids=ids, table=table, **tp)  # (the device's own table)
        got = t.read_denoised()
        t.clear_canvas()
        got_h = t.read_denoise_history()
        t.update_scene(now, tris, mats)
        border = want["rep"]["borderline"]
        with np.errstate(all="ignore"):
            ok = np.isclose(got[..., :3], want["c"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= np.isclose(got[..., 3], want["V"], rtol=1e-4, atol=1e-7, equal_nan=True)
            ok &= np.isclose(got_h["count"], want["commit"]["count"], rtol=1e-4)
            ok &= np.isclose(got_h["m1"], want["commit"]["m1"], rtol=1e-4, atol=1e-6, equal_nan=True)
            ok &= np.isclose(got_h["m2"], want["commit"]["m2"], rtol=1e-4, atol=1e-6, equal_nan=True)
            ok &= np.isclose(got_h["colour"], want["commit"]["colour"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= (np.abs(argb.astype(int) - D.tonemap(want["c"]).astype(int)) <= 1).all(-1)
        bad = ~ok & ~border
        print(f"{name} frame {k}: {int((~ok).sum())} pixels differ ({int(bad.sum())} unflagged), {border.mean() * 100:.3f}% flagged")
        assert not bad.any(), (k, np.argwhere(bad)[:5])
        assert int((~ok & border).sum()) < 1e-3 * w * h, k
        assert border.mean() <= 0.01, k
        on_moved = np.isin(ids, moved_idx)
        kept = on_moved & (want["h"] > 0) & ~border
        lost = (want["cur"]["cov"] > 0) & (want["rep"]["taps"] == 0) & ~border
        assert kept.any() and lost.any(), k
        assert np.all(got_h["count"][kept] > want["cur"]["P"]) and np.all(got_h["count"][lost] == want["cur"]["P"]), k
    t.close()


# ---- 7. state ------------------------------------------------------------------------------------------------------------------
def test_keep_and_drop_rules(T, sky):
    w, h = 64, 40
    shapes, tris, mats = S.mixed_test_scene()
    t = make(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={}, temporal={}, motion=True)

    def commit(scene_shapes=shapes):
        t.update_scene(scene_shapes, tris, mats)
        t.options["time"] += 1
        t.render(1)
        t.clear_canvas()
        assert t.read_denoise_history()["valid"]

    def valid():
        return t.read_denoise_history()["valid"]

    commit()
    same = [np.frombuffer(bytearray(a.tobytes()), a.dtype) for a in (shapes, tris, mats)]
    t.update_scene(*same)
    assert valid() and not t.read_denoise_motion()["any_moved"]
    allowed = [[(1, "translate", (0.1, 0.0, 0.0))], [(5, "scale", 1.1)], [(0, "shift", 0.05)], [(7, "tilt", 0.02)], [(2, "translate", (0.0, 0.1, 0.0))],
               [(4, "rotate", 0.1)], [(6, "scale", 1.05)]]
    for steps in allowed:
        commit()
        t.update_scene(M.move_shapes(shapes, tris, steps, 1), tris, mats)
        assert valid() and t.read_denoise_motion()["state"][steps[0][0]] == M.MOVED, steps
        t.update_scene(M.move_shapes(shapes, tris, steps, 2), tris, mats)  # several updates between two traces: still against the history
        assert valid()
    # a degenerate move keeps the history of the others and gives that shape none
    commit()
    flat = M.move_shapes(shapes, tris, [], 0)
    flat["sphere_radius"][1] = 0.0
    t.update_scene(flat, tris, mats)
    assert valid() and t.read_denoise_motion()["state"][1] == M.NO_HISTORY

    def edit(field, idx, value):
        s = M.move_shapes(shapes, tris, [], 0)
        s[field][idx] = value
        return lambda: t.update_scene(s, tris, mats)

    m2, t2 = mats.copy(), tris.copy()
    m2[0]["smoothness"] = 0.5
    t2["v"]["pos"][20, 0, 0] += 0.5
    sd = t.scene_data.copy()
    drops = [edit("material", 1, 3), edit("num_triangles", 4, 100), lambda: t.update_scene(shapes[:-1], tris, mats), lambda: t.update_scene(shapes, tris, m2),
             lambda: t.update_scene(shapes, t2, mats), lambda: (t.scene_data.__setitem__("sun_intensity", 2.0), t.update_scene(shapes, tris, mats)),
             lambda: t.set_denoise_object_motion(False), lambda: (t.set_denoise_object_motion(False), t.set_denoise_object_motion(True)),
             lambda: t.reset_denoise_history()]
    for i, trig in enumerate(drops):
        t.scene_data = sd.copy()
        t.set_denoise_object_motion(True)
        commit()
        trig()
        assert not valid(), i
    t.scene_data = sd.copy()
    t.set_denoise_object_motion(True)
    # a mixed frame: the scene changes between two dispatches of one frame; that frame does not become a history
    commit()
    t.update_scene(shapes, tris, mats)
    t.render(1)
    t.update_scene(M.move_shapes(shapes, tris, allowed[0], 1), tris, mats)
    t.render(2)
    t.clear_canvas()
    assert not valid()
    t.render(1)
    t.clear_canvas()
    assert valid()  # and the next whole frame does
    t.close()


def test_moved_shape_accumulates_history(T, sky):
    """a sphere dragged for six frames: its pixels end with a history count above one frame's samples"""
    w, h = 96, 54
    shapes, tris, mats = S.sphere_scene()
    t = make(T, sky, (shapes, tris, mats), w, h, denoise={}, temporal={}, motion=True)
    steps = [(4, "translate", (0.03, 0.01, 0.0))]
    for k in range(6):
        t.clear_canvas()
        t.update_scene(M.move_shapes(shapes, tris, steps, k), tris, mats)
        t.options["time"] = 50 + k
        t.render(1)
    ids = t.read_denoise_shape_ids()[0]
    t.clear_canvas()
    count = t.read_denoise_history()["count"]
    on = ids == 4
    assert on.sum() > 20 and np.median(count[on]) >= 10 and abs(count[on].max() - 12) < 1e-4  # (weight-normalised: 12 within rounding)
    t.close()


def test_error_codes(T, sky):
    scn = S.sphere_scene()
    t = make(T, sky, scn, 32, 24)
    for call in (lambda: t.set_denoise_object_motion(True), lambda: t.read_denoise_shape_ids(), lambda: t.read_denoise_motion()):
        with pytest.raises(T.SrtError):
            call()
    t.set_denoise()
    with pytest.raises(T.SrtError):
        t.set_denoise_object_motion(True)  # temporal is off
    t.set_denoise_temporal()
    t.set_denoise_object_motion(True)
    n, moved = __import__("ctypes").c_size_t(0), __import__("ctypes").c_int(0)
    table = np.zeros((2, T.MOTION_WORDS), np.uint32)
    rc = t.lib.srt_read_denoise_motion(t._h, table.ctypes.data, 2, __import__("ctypes").byref(n), __import__("ctypes").byref(moved))
    assert rc == 1 and n.value == len(scn[0])  # SRT_ERR_INVALID: too little room, the count still reported
    with pytest.raises(T.SrtError):
        t.set_partition(0, 2)
    t.set_denoise_temporal(False)  # turns object motion off with it
    with pytest.raises(T.SrtError):
        t.read_denoise_motion()
    t.set_denoise_temporal()
    t.set_denoise_object_motion(True)
    t.set_denoise(False)
    with pytest.raises(T.SrtError):
        t.read_denoise_motion()
    assert t.lib.srt_set_denoise_object_motion(None, 1) == 1
    t.close()


# ---- 8. quality while a shape is dragged --------------------------------------------------------------------------------
def dilate(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= np.roll(np.roll(mask, dy, 0), dx, 1)
    return out


QUALITY = {"spheres": ("spheres", 0, [(4, "translate", (0.05, 0.02, 0.03))]),
           "meshes": ("meshes", 1, [(2, "translate", (-0.04, 0.015, 0.03)), (2, "rotate", 0.04)])}


@pytest.mark.parametrize("name", ["spheres", "meshes"])
def test_quality_dragged_shape(T, sky, name):
    """160x90, 8 frames at 2 spp, default filter, camera still, tonemapped MSE against 4096 spp of the last scene; against
    the spatial filter alone, which is what the library delivers in this situation without object motion (asserted). Measured
    (profiles/r07_motion_quality.json): see DESIGN.md section 12."""
    scn_name, accel, steps = QUALITY[name]
    w, h, frames = 160, 90, 8
    shapes, tris, mats = scene(scn_name)
    idx = steps[0][0]

    def at(k):
        s = shapes
        for st in steps:  # a translation and a rotation of one model compose
            s = M.move_shapes(s, tris, [st], k)
        return s

    g = make(T, sky, (at(frames - 1), tris, mats), w, h, spp=4096, accel=accel, time=4242)
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    sp = make(T, sky, (shapes, tris, mats), w, h, accel=accel, denoise={})
    off = make(T, sky, (shapes, tris, mats), w, h, accel=accel, denoise={}, temporal={})
    om = make(T, sky, (shapes, tris, mats), w, h, accel=accel, denoise={}, temporal={}, motion=True)
    covered = np.zeros((h, w), bool)
    for k in range(frames):
        for t in (sp, off, om):
            t.clear_canvas()
            t.update_scene(at(k), tris, mats)
            t.options["time"] = 900 + k
            t.render(1)
        if k:
            assert not off.read_denoise_history()["valid"] and om.read_denoise_history()["valid"], k
        ids = om.read_denoise_shape_ids()[0]
        covered |= ids == idx
    a, b, c = (t.read_denoised()[..., :3] for t in (sp, off, om))
    assert bits_equal(a, c) is False and bits_equal(a, b)  # without object motion a dragged shape means the spatial filter every frame
    on = ids == idx
    near = dilate(covered, 8) & ~on
    mse = lambda x, m: float(np.mean((tone(x)[m] - ref[m]) ** 2))
    everything = np.ones((h, w), bool)
    ratios = {k: mse(c, m) / mse(a, m) for k, m in (("image", everything), ("moved_shape", on), ("around", near))}
    print(f"motion quality {name}: " + json.dumps({**ratios, "moved_pixels": int(on.sum()), "around_pixels": int(near.sum()),
                                                   "mse_spatial": mse(a, everything), "mse_motion": mse(c, everything)}))
    for t in (sp, off, om):
        t.close()
    assert on.sum() > 50 and near.sum() > 50
    assert ratios["image"] < 1.0 and ratios["moved_shape"] < 1.0  # the criterion: better than what the library gave before
    # regression guard, about twice the measured 0.27 / 0.14 (spheres) and 0.34 / 0.30 (meshes); runs are bit-identical
    assert ratios["image"] < 0.7 and ratios["moved_shape"] < 0.6
    assert ratios["around"] < 1.25
