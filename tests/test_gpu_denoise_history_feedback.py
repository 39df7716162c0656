"""GPU: the history feedback (srt_set_denoise_history_feedback). The colour a clear commits against the numpy
restatement (tests/feedback_ref.py) one frame at a time from the device's own previous history; that only the colour changes;
that untouched pixels keep their bits; that the history does not depend on whether a filter ran; off is off; the frame's own
output is unchanged; repeats; the other temporal switches; a device group; the switch's rules; srt_headless; and that a still
camera converges to the spatial filter's image."""
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import feedback_ref as FB
import motion_ref as M
import temporal_cases as TC
from conftest import bits_equal
from gpu_harness import T, cam_at, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
SRT_ERR_INVALID, SRT_ERR_STATE = 1, 3
TP = dict(history_limit=32, normal_threshold=0.9, depth_threshold=0.05)
FRAMES = [("spheres", 0, 128, 72), ("spheres", 0, 37, 29), ("mixed", 1, 128, 72), ("spheres", 0, 33, 1), ("spheres", 0, 1, 33)]
FRAME_IDS = [f"{s}-{w}x{h}" for s, _, w, h in FRAMES]
MODES = [(K, demod, ms) for K in (1, 5) for demod in (False, True) for ms in (0, 8)]
MODE_IDS = [f"K{K}-{'demod' if d else 'plain'}-sv{ms}" for K, d, ms in MODES]
SETS = ("colour", "count", "m1", "m2", "guide")


def handle(T, sky, scn, w, h, K=5, fb=True, demod=False, ms=0, gamma=0.0, illum=False, motion=False, accel=0, group=0, cam=None, time=31, **dn):
    """a tracer over scn, 2 spp, the denoiser with K passes, temporal reprojection and the switches as given; group > 0: a
    TracerGroup of that many virtual devices"""
    shapes, tris, mats = scene(scn) if isinstance(scn, str) else scn
    dn = dict(iterations=K, **dn)
    if group:
        t = T.TracerGroup(w, h, n_devices=group, devices=[0] * group, rows_per_block=8)
        t.set_skybox(sky)
        t.set_acceleration(accel)
        t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera() if cam is None else cam, time=time)
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        t.set_denoise(**dn)
        t.set_denoise_temporal(**TP)
        t.scene = (shapes, tris, mats)
    else:
        t = make(T, sky, (shapes, tris, mats), w, h, spp=2, accel=accel, time=time, cam=cam, denoise=dn, temporal=TP, motion=motion)
    if demod:
        t.set_denoise_demodulation(True)
    if ms:
        t.set_denoise_spatial_variance(ms)
    if illum:
        t.set_denoise_history_illumination(True)
    if gamma:
        t.set_denoise_history_clamp(gamma)
    if fb:
        t.set_denoise_history_feedback(True)
    return t


def same_history(a, b, keys=SETS):
    assert a["valid"] == b["valid"]
    for k in keys:
        assert bits_equal(a[k], b[k]), k


def aim(t, k, kind="move", scn=None, time=None):
    """frame k of a moving sequence: the scene again (as the front-end does), the camera, the seed"""
    t.update_scene(*(t.scene if scn is None else scn))
    if kind is not None:
        t.options["camera_to_world"] = cam_at(k, kind)
    t.options["time"] = 700 + k if time is None else time


def next_frame(t, k, kind="move", scn=None):
    t.clear_canvas()
    aim(t, k, kind, scn)
    return t.render(1).copy()


def adopt_setup(want, dev, got, label):
    """§11's and §20's rule for a set-up against numpy, then the device's own values where that rule lets them differ. dev = the
    set-up's {colour, variance} (a filter of the same frame with K = 0), got = the committed history. Off the pixels the
    reprojection's restatement flags as decided by a rounding (at most 1 % of a frame) and the ones it clamps (whose bounds come
    from fast exp / log), colour, variance, count and moments agree bit for bit; a clamped pixel that is not flagged agrees within
    rtol 1e-4. Those pixels then take the device's values, so that pass 1 is compared over the inputs it had."""
    rep, commit = want["rep"], want["commit"]
    border = rep["borderline"]
    loose = border | rep.get("clamped", np.zeros(border.shape, bool))
    assert got["valid"] and border.mean() <= 0.01, label
    assert bits_equal(got["guide"], commit["guide"]), label
    pairs = [(dev[..., :3], want["c"], 1e-6), (dev[..., 3], want["V"], 1e-7), (got["count"], commit["count"], 0.0), (got["m1"], commit["m1"], 1e-6),
             (got["m2"], commit["m2"], 1e-6)]
    same, close = np.ones(border.shape, bool), np.ones(border.shape, bool)
    with np.errstate(all="ignore"):
        for x, y, atol in pairs:
            same &= TC.same_bits(x, y)
            ok = np.isclose(x, y, rtol=1e-4, atol=atol, equal_nan=True)
            close &= ok.reshape(ok.shape[:2] + (-1,)).all(-1)
    assert not (~same & ~loose).any(), (label, np.argwhere(~same & ~loose)[:5])
    assert not (~close & ~border).any(), (label, np.argwhere(~close & ~border)[:5])
    c, V = np.where(loose[..., None], dev[..., :3], want["c"]).astype(np.float32), np.where(loose, dev[..., 3], want["V"]).astype(np.float32)
    staged = dict(commit, colour=c.copy(), **{k: np.where(loose, got[k], commit[k]).astype(np.float32) for k in ("count", "m1", "m2")})
    return dict(want, c=c, V=V, commit=staged), int(loose.sum()), int((~same).sum())


def check_commit(want, dev, got, label, K, demod, ms, sigmas=None):
    """the history a clear committed (got) against the restatement: count, moments and guide bit for bit (adopt_setup's rule), the
    colour against feedback_ref.feed_back over the set-up at rtol 1e-4, atol 1e-6, the project's tolerance for a pass against numpy
    (test_filter_matches_numpy), on every pixel; a pixel the restatement does not write keeps the set-up's colour bit for bit."""
    st, loose, differ = adopt_setup(want, dev, got, label)
    fbk = FB.feed_back(st, K, demod=demod, min_samples=ms, **(sigmas or {}))
    for k in ("count", "m1", "m2"):
        assert bits_equal(got[k], fbk[k]), (label, k)
    with np.errstate(all="ignore"):
        ok = np.isclose(got["colour"], fbk["colour"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
        err = np.abs(got["colour"] - fbk["colour"]) / (np.abs(fbk["colour"]) + 1e-2)
    print(f"{label}: {int(fbk['written'].sum())} of {ok.size} pixels written, {loose} pixels flagged or clamped ({differ} differ in a bit from the "
          f"restatement's set-up), worst colour error {np.nanmax(err):.2e}")
    assert ok.all(), (label, np.argwhere(~ok)[:5])
    kept = ~fbk["written"]
    assert TC.same_bits(got["colour"], st["commit"]["colour"])[kept].all(), label
    return fbk, st


def run_parity(t, frames, label, K, demod=False, ms=0, kind="move", moves=None, **ref_kw):
    """frames 2-spp frames with a clear between them; each committed history against the restatement fed the device's previous one"""
    written = changed = 0
    for k in range(frames):
        t.clear_canvas()
        hist = t.read_denoise_history()
        scn = None
        if moves is not None:
            hist["ids"] = t.read_denoise_shape_ids()[1]
            scn = (M.move_shapes(t.scene[0], t.scene[1], moves, k), t.scene[1], t.scene[2])
        aim(t, k, kind, scn)
        if moves is not None:
            ref_kw["table"] = t.read_denoise_motion()
        t.render(1)
        assert t.last_filter_history_feedback()
        t.set_denoise(iterations=0)  # the set-up's own output: a filter of the same frame without a pass
        t.resolve_denoised(1)
        assert not t.last_filter_history_feedback()
        dev = t.read_denoised()
        t.set_denoise(iterations=K)
        t.resolve_denoised(1)  # (and a repeated filter stages what one stages)
        inp = t.read_denoise_inputs()
        if moves is not None:
            ref_kw["ids"] = t.read_denoise_shape_ids()[0]
        want = FB.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, iterations=K, demod=demod, min_samples=ms, **ref_kw, **TP)
        t.clear_canvas()
        fbk, st = check_commit(want, dev, t.read_denoise_history(), f"{label} frame {k}", K, demod, ms)
        if moves is not None:
            t.update_scene(*scn)
        written += int(fbk["written"].sum())
        changed += int((~TC.same_bits(fbk["colour"], st["commit"]["colour"])).sum())
    assert written > 0 and changed > 0, label  # (the restatement itself says the switch-off history is another one)


# ---- 1. one-step parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,demod,ms", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("scn,accel,w,h", FRAMES, ids=FRAME_IDS)
def test_committed_colour_matches_numpy(T, sky, scn, accel, w, h, K, demod, ms):
    t = handle(T, sky, scn, w, h, K=K, demod=demod, ms=ms, accel=accel, cam=cam_at(0, "move"))
    run_parity(t, 3, f"{scn} {w}x{h} K={K} demod={demod} sv={ms}", K, demod, ms)
    t.close()


# ---- 2., 3. only the colour changes; untouched pixels -------------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [False, True])
def test_only_the_colour_changes(T, sky, demod):
    """over the nan scene of tests/temporal_cases.py (a material whose colour is NaN) without its back wall (so the sky shows above
    the floor): count, moments and guide of every
    committed history equal the switch-off handle's bit for bit; so does the colour of every sky pixel and every pixel whose
    colour is not finite; the other pixels' colours do differ"""
    w, h = 128, 72
    shapes, tris, mats = TC.nan_scene()
    open_scene = (shapes[[0, 1, 3, 4, 5, 6]], tris, mats)
    on, off = (handle(T, sky, open_scene, w, h, fb=f, demod=demod) for f in (True, False))
    for k in range(4):
        for t in (on, off):
            next_frame(t, k)
        assert on.last_filter_history_feedback() and not off.last_filter_history_feedback()
        for t in (on, off):
            t.clear_canvas()
        a, b = on.read_denoise_history(), off.read_denoise_history()
        same_history(a, b, ("count", "m1", "m2", "guide"))
        sky_px = a["guide"][..., 1, 3] == 0
        nan_px = ~np.isfinite(b["colour"]).all(-1)
        assert sky_px.any() and nan_px.any() and (nan_px & ~sky_px).any()
        eq = TC.same_bits(a["colour"], b["colour"])
        assert eq[sky_px | nan_px].all(), k
        assert (~eq[~(sky_px | nan_px)]).mean() > 0.5, k
    on.close()
    off.close()


# ---- 4. filter or no filter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,demod,ms", [(1, False, 0), (1, True, 0), (5, False, 8), (5, True, 8)])
def test_the_history_does_not_depend_on_whether_a_filter_ran(T, sky, K, demod, ms):
    w, h = 64, 48
    a, b = (handle(T, sky, "spheres", w, h, K=K, demod=demod, ms=ms) for _ in range(2))
    for k in range(3):
        for t in (a, b):
            aim(t, k)
        a.render(1)
        b.trace()
        argb = b.read_argb().copy()
        for t in (a, b):
            t.clear_canvas()
            assert t.last_filter_history_feedback()
        assert np.array_equal(b.read_argb(), argb)  # the clear's own pass writes no ARGB image
        with pytest.raises(T.SrtError):
            b.read_denoised()  # and it used the filter's images
        assert T.load_library().srt_read_denoised(b._h, np.zeros((h, w, 4), np.float32).ctypes.data) == SRT_ERR_STATE
        a.read_denoised()
        same_history(a.read_denoise_history(), b.read_denoise_history())
    a.close()
    b.close()


@pytest.mark.parametrize("change", ["sigma", "iterations", "demodulation", "spatial_variance", "switch_off", "switch_on"])
def test_a_setter_between_the_filter_and_the_clear(T, sky, change):
    """filter, change a setting pass 1 depends on, clear: the clear commits what a handle commits that had the setting all along"""
    w, h = 64, 48
    start_fb = change != "switch_on"
    a, b = (handle(T, sky, "spheres", w, h, K=3, fb=start_fb) for _ in range(2))

    def apply(t):
        if change == "sigma":
            t.set_denoise(iterations=3, sigma_luminance=1.0)
        elif change == "iterations":
            t.set_denoise(iterations=1)
        elif change == "demodulation":
            t.set_denoise_demodulation(True)
        elif change == "spatial_variance":
            t.set_denoise_spatial_variance(8)
        else:
            t.set_denoise_history_feedback(change == "switch_on")

    for t in (a, b):
        next_frame(t, 0)
    for t in (a, b):
        t.clear_canvas()
        aim(t, 1)
    a.render(1)  # a filters with the old setting, then changes it
    apply(a)
    apply(b)  # b changes it first and only traces
    b.trace()
    for t in (a, b):
        t.clear_canvas()
    assert a.last_filter_history_feedback() == b.last_filter_history_feedback()
    same_history(a.read_denoise_history(), b.read_denoise_history())
    a.close()
    b.close()


# ---- 5. off is off --------------------------------------------------------------------------------------------------------------------
def test_off_is_off(T, sky):
    """never touched, turned on and off again, on with K = 0: the same bytes and histories; on with K = 2: another history"""
    w, h = 64, 48
    never = handle(T, sky, "spheres", w, h, K=2, fb=False)
    off = handle(T, sky, "spheres", w, h, K=2)
    off.set_denoise_history_feedback(False)
    on = handle(T, sky, "spheres", w, h, K=2)
    never0, on0 = handle(T, sky, "spheres", w, h, K=0, fb=False), handle(T, sky, "spheres", w, h, K=0)
    for k in range(3):
        outs = {t: next_frame(t, k) for t in (never, off, on, never0, on0)}
        assert np.array_equal(outs[never], outs[off]) and bits_equal(never.read_denoised(), off.read_denoised()), k
        assert np.array_equal(outs[never0], outs[on0]) and bits_equal(never0.read_denoised(), on0.read_denoised()), k
        assert [t.last_filter_history_feedback() for t in (never, off, on, never0, on0)] == [False, False, True, False, False]
    for t in (never, off, on, never0, on0):
        t.clear_canvas()
    same_history(never.read_denoise_history(), off.read_denoise_history())
    same_history(never0.read_denoise_history(), on0.read_denoise_history())
    assert not bits_equal(never.read_denoise_history()["colour"], on.read_denoise_history()["colour"])
    on0.trace()
    on0.clear_canvas()  # K = 0: the clear runs the set-up alone
    assert not on0.last_filter_history_feedback()
    for t in (never, off, on, never0, on0):
        t.close()


# ---- 6., 7. the frame's own output; repeats --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [False, True])
def test_same_frame_output_unchanged_and_repeats(T, sky, demod):
    w, h = 64, 48
    on, off, twin, once = (handle(T, sky, "spheres", w, h, fb=f, demod=demod, ms=8) for f in (True, False, True, True))
    for t in (on, off, twin, once):
        next_frame(t, 0)
        next_frame(t, 1)
    outs = []
    for t in (on, off, twin, once):  # all start again from no history (dropped after the clear's commit): the frame's inputs are the same
        t.clear_canvas()
        t.reset_denoise_history()
        aim(t, 2)
        outs.append(t.render(1).copy())
    assert np.array_equal(outs[0], outs[1]) and bits_equal(on.read_denoised(), off.read_denoised())
    # and from one history: the second handle gives the switch up only now, and its frame is the first handle's
    a = next_frame(on, 3)
    twin.clear_canvas()  # (the commit first: a change of the switch before it would make the clear stage the switch-off colour)
    twin.set_denoise_history_feedback(False)
    aim(twin, 3)
    b = twin.render(1).copy()
    assert not twin.last_filter_history_feedback()
    assert np.array_equal(a, b) and bits_equal(on.read_denoised(), twin.read_denoised())
    # a second filter of the frame: the same bytes, and the same commit as one
    first = on.read_denoised()
    on.resolve_denoised(1)
    assert np.array_equal(on.read_argb().ravel(), a.ravel()) and bits_equal(on.read_denoised(), first)
    next_frame(once, 3)
    for t in (on, once):
        t.clear_canvas()
    same_history(on.read_denoise_history(), once.read_denoise_history())
    for t in (on, off, twin, once):
        t.close()


# ---- 8. the other temporal switches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["clamp", "illumination", "motion"])
def test_combinations_match_numpy(T, sky, combo):
    w, h = 96, 64
    if combo == "clamp":
        t = handle(T, sky, "spheres", w, h, K=5, gamma=1.0, cam=cam_at(0, "move"))
        run_parity(t, 3, "clamp", 5, gamma=1.0)
        assert t.last_setup_history_clamp()
    elif combo == "illumination":
        t = handle(T, sky, "mixed", w, h, K=5, demod=True, illum=True, accel=1, cam=cam_at(0, "move"))
        run_parity(t, 3, "illumination", 5, demod=True, rescale=True)
        assert t.last_setup_history_illumination()
    else:
        t = handle(T, sky, "spheres", w, h, K=5, motion=True)
        run_parity(t, 3, "motion", 5, kind=None, moves=[(4, "translate", (0.05, 0.02, 0.03))])
    t.close()


# ---- 9. a device group --------------------------------------------------------------------------------------------------------------------
def test_group_equals_the_single_handle(T, sky):
    w, h = 48, 40
    single, group = (handle(T, sky, "spheres", w, h, K=2, demod=True, group=g) for g in (0, 3))
    for k in range(3):
        outs = [next_frame(t, k, "yaw") for t in (single, group)]
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(single.read_denoised(), group.read_denoised()), k
        assert single.last_filter_history_feedback() and group.last_filter_history_feedback()
    for t in (single, group):
        t.clear_canvas()
    same_history(single.read_denoise_history(), group.read_denoise_history())
    for t in (single, group):  # trace alone, a setter, then the clear's own front
        aim(t, 3, "yaw")
        t.trace() if t is single else t.trace_and_gather()
        t.set_denoise_demodulation(False)
        t.clear_canvas()
    same_history(single.read_denoise_history(), group.read_denoise_history())
    lib = T.load_library()
    group.set_denoise_temporal(False)
    assert lib.srt_group_set_denoise_history_feedback(group._g, 1) == SRT_ERR_STATE  # the group's temporal reprojection is off
    assert lib.srt_group_set_denoise_history_feedback(group._g, 0) == 0
    single.close()
    group.close()


# ---- 10. the switch's rules ---------------------------------------------------------------------------------------------------------------
def test_state_rules(T, sky):
    lib = T.load_library()
    w, h = 48, 32
    t = make(T, sky, "spheres", w, h)
    assert lib.srt_set_denoise_history_feedback(t._h, 1) == SRT_ERR_STATE  # the denoiser is off
    assert lib.srt_set_denoise_history_feedback(t._h, 0) == 0
    t.set_denoise(iterations=2)
    assert lib.srt_set_denoise_history_feedback(t._h, 1) == SRT_ERR_STATE  # temporal reprojection is off
    with pytest.raises(T.SrtError):
        t.set_denoise_history_feedback()
    t.set_denoise_temporal()
    t.set_denoise_history_feedback()
    t.render(1)
    assert t.last_filter_history_feedback()
    t.clear_canvas()
    before = t.read_denoise_history()
    t.set_denoise_history_feedback(False)
    t.set_denoise_history_feedback(True)
    same_history(before, t.read_denoise_history())  # toggling clears nothing
    t.set_denoise_temporal(history_limit=16)  # another setting of the temporal stage: the switch stays
    t.render(1)
    assert t.last_filter_history_feedback()
    t.set_denoise_temporal(False)  # turning temporal off turns it off
    t.set_denoise_temporal()
    t.render(2)
    assert not t.last_filter_history_feedback()
    t.set_denoise_history_feedback()
    t.set_denoise(False)  # and so does turning the denoiser off
    t.set_denoise(iterations=2)
    t.set_denoise_temporal()
    t.render(1)
    assert not t.last_filter_history_feedback()
    t.close()
    p = T.Tracer(w, h)
    p.set_partition(0, 2)
    assert lib.srt_set_denoise_history_feedback(p._h, 1) == SRT_ERR_STATE  # never on a partitioned handle
    p.close()
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=8)
    assert lib.srt_group_set_denoise_history_feedback(g._g, 1) == SRT_ERR_STATE  # no denoiser yet
    assert lib.srt_group_set_denoise_history_feedback(g._g, 0) == 0
    assert not g.last_filter_history_feedback()
    g.close()
    for e in (0, 1):
        assert lib.srt_set_denoise_history_feedback(None, e) == SRT_ERR_INVALID and lib.srt_group_set_denoise_history_feedback(None, e) == SRT_ERR_INVALID
    assert lib.srt_last_filter_history_feedback(None) == 0 and lib.srt_group_last_filter_history_feedback(None) == 0


# ---- 11. srt_headless -----------------------------------------------------------------------------------------------------------------------
def test_headless_history_feedback_writes_another_second_frame(tmp_path):
    """a frame without a history is the same picture with the switch; the second frame of a history's sequence is another one. The
    tool's history starts with its second frame (its first update_scene carries another scene record than the later ones, which
    drops the history once), so --frames 2 has no history yet and --frames 3 is that second frame"""
    from simple_raytracer_amd import build
    exe = build.build_headless()
    out = {}
    for frames in (2, 3):
        for extra in ((), ("--history-feedback",)):
            f = tmp_path / f"f{frames}{len(extra)}.ppm"
            subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", str(frames), "--denoise", "5",
                            "--temporal", "--move", "0.02", "--out", str(f), *extra], check=True, timeout=120)
            out[frames, bool(extra)] = f.read_bytes()
    assert out[3, True].startswith(b"P6") and len(out[3, True]) == len(out[3, False]) > 64 * 48 * 3
    assert out[2, True] == out[2, False]
    assert out[3, True] != out[3, False]


# ---- quality ----------------------------------------------------------------------------------------------------------------------------------
# Measured on an MI355X by scripts/history_feedback_probe.py (profiles/r24_history_feedback_quality.json): the tonemapped MSE of
# the eighth 2-spp frame of the moving camera against 4096 spp, switch on over switch off, the worst of three seeds. None: no
# claim is made for the scene and nothing is asserted about its ratio.
# Measured: spheres 1.105 / 1.122 / 1.124 (demodulated 1.080 / 1.106 / 1.105), meshes 1.167 / 1.178 / 1.197 (demodulated 1.156 / 1.177 /
# 1.192): the feedback is worse on every seed, so neither scene earns a claim. (The noise-textured scene: 1.06 alone, 1.01 with
# demodulation and history illumination.)
WORST_RATIO = {"spheres": None, "meshes": None}


@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 1)])
def test_quality_and_preservation(T, sky, name, accel):
    """the set-up of test_quality_moving_camera (tests/test_gpu_denoise_temporal.py). The ratio is printed, and asserted only where
    a claim was earned (a worst measured ratio of at most 0.85: then at most that x 1.15, seed to seed). Preservation is asserted
    always: after the camera stops and the canvas reaches 1024 samples, the switch-on frame against the spatial filter's is at least
    40 dB, the bar that test sets for the temporal stage."""
    w, h, frames = 160, 90, 8
    g = make(T, sky, name, w, h, spp=4096, accel=accel, time=4242)
    g.options["camera_to_world"] = cam_at(frames - 1, "move")
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    sp = make(T, sky, name, w, h, accel=accel, denoise={})
    off = make(T, sky, name, w, h, accel=accel, denoise={}, temporal={})
    on = make(T, sky, name, w, h, accel=accel, denoise={}, temporal={})
    on.set_denoise_history_feedback()
    for k in range(frames):
        for t in (sp, off, on):
            t.clear_canvas()
            aim(t, k, time=900 + k)
            t.render(1)
    mse = {t: float(np.mean((tone(t.read_denoised()[..., :3]) - ref) ** 2)) for t in (sp, off, on)}
    ratio = mse[on] / mse[off]
    print(f"{name}: spatial MSE {mse[sp]:.3e}, temporal {mse[off]:.3e}, with the feedback {mse[on]:.3e}: ratio {ratio:.3f}")
    if WORST_RATIO[name] is not None:
        assert WORST_RATIO[name] <= 0.85 and ratio <= WORST_RATIO[name] * 1.15
    for t in (sp, on):
        for i in range(1, 512):
            t.options["time"] = 7000 + i
            if i < 511:
                t.trace()
            else:
                t.render(i + 1)
    p = D.psnr(tone(on.read_denoised()[..., :3]), tone(sp.read_denoised()[..., :3]))
    print(f"{name}: after the camera stopped, feedback vs spatial at 1024 spp: {p:.1f} dB")
    assert p >= 40.0
    for t in (sp, off, on):
        t.close()
