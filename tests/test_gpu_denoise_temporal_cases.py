"""GPU: the temporal set-up under a moved camera (TP_PROJECT of srt_temporal_kernel, csrc/temporal.hip) at its edges -- the cases of
tests/temporal_cases.py (zoom, aspect, roll, large turns, an about-face, scaled, mirrored, sheared and singular cameras) on
whole and ragged frames, two thresholds pairs and three scenes, the cap at history_limit under projection, frames of two
dispatches and of another sample count than their history, a history with non-finite colours, and the moved kernel.

Every frame is compared with tests/temporal_ref.py fed the device's own canvas, inputs and history: bit for bit on the
pixels the restatement does not flag `borderline`, within rtol 1e-4 on those, of which fewer than 0.1 % of the frame may
differ. tests/test_temporal_cases.py holds the restatement alone to the cases' flagged shares and branches on the CPU."""
import numpy as np
import pytest

import motion_ref as M
import temporal_cases as TC
import temporal_ref as TR
from conftest import bits_equal
from gpu_harness import T, make, scene  # noqa: F401 (T: the fixture)

pytestmark = pytest.mark.gpu

FRAMES = [(128, 72), (37, 29), (1, 33), (33, 1)]  # whole 16x16 tiles across; ragged both ways; one column; one row
THRESHOLDS = [(0.9, 0.05), (-1.0, 10.0)]  # the defaults; every tap in the image with coverage and a finite colour counts
SCENES = [("mixed", 0), ("mixed", 1), ("spheres", 0)]


@pytest.fixture(scope="module")
def pool(T, sky):
    """tracers by (scene, acceleration, width, height, object motion), made once: a test starts from fresh()"""
    made = {}

    def get(scn, accel, w, h, motion=False):
        key = (scn, accel, w, h, motion)
        if key not in made:
            arrays = TC.nan_scene() if scn == "nan" else scene(scn)
            made[key] = make(T, sky, arrays, w, h, accel=accel, denoise=dict(iterations=0), temporal={}, motion=motion)
        return made[key]

    yield get
    for t in made.values():
        t.close()


def fresh(t, tp):
    """no history, nothing traced, the scene as made, the thresholds tp"""
    t.clear_canvas()
    t.reset_denoise_history()
    t.update_scene(*t.scene)
    t.set_denoise_temporal(**tp)
    assert not t.read_denoise_history()["valid"]


def aim(t, cam, spp=2):
    m, fov, aspect = cam
    t.options["camera_to_world"] = m
    t.options["fov_scale"] = fov
    t.options["aspect_ratio"] = np.float32(t.width) / np.float32(t.height) if aspect is None else aspect
    t.options["num_samples"] = spp


def history(t, motion=False):
    hist = t.read_denoise_history()
    if motion:
        hist["ids"] = t.read_denoise_shape_ids()[1]
    return hist


def check_frame(t, hist, tp, argb, label, ids=None, table=None):
    """the frame just rendered against the restatement, then the clear and the history it commits. -> (want, read_denoised(), that history)"""
    w, h = t.width, t.height
    inp = t.read_denoise_inputs()
    want = TR.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, ids=ids, table=table, **tp)
    got = t.read_denoised()
    t.clear_canvas()
    got_h = t.read_denoise_history()
    assert got_h["valid"] and got_h["camera"].tobytes() == t.options.tobytes()
    exact, close, worst = TC.compare_setup(want, got, argb.reshape(h, w, 4), got_h)
    border = want["rep"]["borderline"]
    print(f"{label} {w}x{h}: {int(border.sum())} pixels flagged ({border.mean() * 100:.3f} %), {int((~exact).sum())} differ in a bit "
          f"({int((~exact & ~border).sum())} unflagged, at most {worst:.1f} ulp), {int((~close).sum())} beyond rtol 1e-4; "
          f"{int((want['h'] > 0).sum())} pixels with history")
    bad = ~exact & ~border
    assert not bad.any(), (label, np.argwhere(bad)[:5])
    assert not (~close & ~border).any()
    assert int((~close & border).sum()) < 1e-3 * w * h, label
    return want, got, got_h


def two_frames(t, hist_cam, cur_cam, tp, label, dispatches=1, spp=2, steps=None):
    """the protocol: a 2-spp frame at the history camera, clear, the history read back, update_scene (the same bytes, or the
    scene moved by `steps` under object motion), the current camera, a frame of `dispatches` dispatches at `spp`"""
    motion = steps is not None
    fresh(t, tp)
    aim(t, hist_cam)
    t.options["time"] = 2000
    t.render(1)
    t.clear_canvas()
    hist = history(t, motion)
    assert hist["valid"]
    shapes, tris, mats = t.scene
    ids = table = None
    if motion:
        t.update_scene(M.move_shapes(shapes, tris, steps, 1), tris, mats)
        table = t.read_denoise_motion()
        assert table["any_moved"]  # srt_temporal_kernel<1, ...> runs
    else:
        t.update_scene(*t.scene)
    assert t.read_denoise_history()["valid"]
    aim(t, cur_cam, spp)
    for d in range(dispatches):
        t.options["time"] = 2001 + d
        argb = t.render(d + 1).copy()
    if motion:
        ids = t.read_denoise_shape_ids()[0]
    want, got, got_h = check_frame(t, hist, tp, argb, label, ids=ids, table=table)
    assert want["cur"]["P"] == dispatches * spp
    want["device"] = got
    return want, got_h, hist, ids


# ---- (a), (b) every case, frame, thresholds pair and scene --------------------------------------------------------------
@pytest.mark.parametrize("scn,accel", SCENES)
@pytest.mark.parametrize("nt,dt", THRESHOLDS)
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("name", TC.NAMES)
def test_case_matches_numpy(pool, name, w, h, nt, dt, scn, accel):
    tp = dict(history_limit=64, normal_threshold=nt, depth_threshold=dt)
    t = pool(scn, accel, w, h)
    hist_cam, cur_cam = TC.CASES[name]
    want, got_h, hist, _ = two_frames(t, hist_cam, cur_cam, tp, f"{name} {scn}/{accel} ({nt}, {dt})")
    covered = want["cur"]["cov"] > 0
    if name in TC.NO_HISTORY:
        assert not (want["h"] > 0).any()
        got = want["device"]
        if name == "hist_singular":  # TP_NONE on the host: the spatial set-up
            assert TR.invert_rotation(hist["camera"]) is None
        assert bits_equal(got[..., :3], want["cur"]["c"]) and bits_equal(got[..., 3], want["cur"]["V"])
        assert np.all(got_h["count"] == want["cur"]["P"])
    elif (w, h) in TC.SIZES:
        assert (want["h"] > 0).any()
        assert nt < 0 or ((want["rep"]["taps"] == 0) & covered).any()  # disoccluded pixels under the default thresholds
        if nt < 0:  # nothing but the image's border, coverage and the colour rejects: the 2x2's that hang over the border
            win = TC.window(want["cur"], hist["camera"], t.options)
            over = (win["x0"] == -1) | (win["x0"] == w - 1) | (win["y0"] == -1) | (win["y0"] == h - 1)
            assert not TC.sees_past_the_border(name, w, h) or (over & (want["h"] > 0)).any()


# ---- (c) the cap at history_limit under projection ------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", TC.SIZES)
def test_cap_is_reached_under_projection(pool, w, h):
    """six 2-spp frames along `dolly` with history_limit 5, then one with the limit lowered to 3 over the same history"""
    tp = dict(history_limit=5, normal_threshold=0.9, depth_threshold=0.05)
    t = pool("mixed", 1, w, h)
    fresh(t, tp)
    hist = dict(valid=False)
    capped = fractional = above = False
    for k in range(7):
        if k == 6:
            tp = dict(tp, history_limit=3)
            t.set_denoise_temporal(**tp)  # on -> on: the history stays
        t.update_scene(*t.scene)
        aim(t, TC.interpolate("dolly", k if k < 6 else 4, 5))  # (the last frame steps back: another camera than its history's)
        t.options["time"] = 3000 + k
        argb = t.render(1).copy()
        want, _, hist = check_frame(t, hist, tp, argb, f"dolly frame {k}")
        hh, lim = want["h"], tp["history_limit"]
        assert hh.max() <= lim
        if k < 6:
            capped |= bool((hh == 5).any())
            fractional |= bool(((hh > 0) & (hh < 5) & (hh != np.floor(hh))).any())
        else:
            above = bool((want["rep"]["h"] > 3).any() and (hh == 3).any())
    assert capped and fractional and above


# ---- (d) a frame of two dispatches, and of another sample count than its history -----------------------------------------
@pytest.mark.parametrize("dispatches,spp", [(2, 2), (1, 3)])
@pytest.mark.parametrize("w,h", TC.SIZES)
@pytest.mark.parametrize("name", ["zoom_in", "roll"])
def test_other_sample_counts_than_the_history(pool, name, w, h, dispatches, spp):
    tp = dict(history_limit=64, normal_threshold=0.9, depth_threshold=0.05)
    t = pool("mixed", 1, w, h)
    want, got_h, _, _ = two_frames(t, *TC.CASES[name], tp, f"{name} T={dispatches} spp={spp}", dispatches=dispatches, spp=spp)
    assert want["cur"]["P"] == dispatches * spp != 2
    has = want["h"] > 0
    assert has.any() and np.all(got_h["count"][has & ~want["rep"]["borderline"]] > want["cur"]["P"])


# ---- (e) a history with non-finite colours next to finite ones ------------------------------------------------------------
@pytest.mark.parametrize("w,h", TC.SIZES)
def test_non_finite_history_colours(pool, w, h):
    tp = dict(history_limit=64, normal_threshold=0.9, depth_threshold=0.05)
    t = pool("nan", 0, w, h)
    want, _, hist, _ = two_frames(t, *TC.CASES["dolly"], tp, "dolly, a NaN material")
    assert not np.isfinite(hist["colour"]).all() and np.isfinite(hist["colour"]).any()
    taps, lost = TC.taps_lost_to_colour(want["cur"], hist, t.options, normal_threshold=0.9, depth_threshold=0.05)
    assert ((lost >= 1) & (lost <= 3) & (taps >= 1)).any()


# ---- (f) the moved kernel under these cameras -------------------------------------------------------------------------------
@pytest.mark.parametrize("scn,accel,steps", [("spheres", 0, [(4, "translate", (0.031, 0.012, 0.02))]),
                                             ("mixed", 1, [(1, "translate", (0.023, 0.0, 0.014))])], ids=["spheres", "mixed-bvh"])
@pytest.mark.parametrize("w,h", TC.SIZES)
@pytest.mark.parametrize("name", ["zoom_in", "roll", "hist_scaled"])
def test_moved_kernel_matches_numpy(pool, name, w, h, scn, accel, steps):
    tp = dict(history_limit=64, normal_threshold=0.9, depth_threshold=0.05)
    t = pool(scn, accel, w, h, motion=True)
    want, got_h, _, ids = two_frames(t, *TC.CASES[name], tp, f"{name} {scn}, a shape moved", steps=steps)
    on_moved = np.isin(ids, [s[0] for s in steps])
    assert "state" in want["rep"] and (want["rep"]["state"][on_moved] == M.MOVED).all()  # the restatement took the table's path
    kept = on_moved & (want["h"] > 0)
    assert kept.any() and (~on_moved & (want["h"] > 0)).any()
