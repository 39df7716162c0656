"""CPU: the history reprojected as illumination (include/srt_abi.h srt_set_denoise_history_illumination). The
numpy restatement tests/history_illumination_ref.py -- which tests/test_gpu_denoise_history_illumination.py pins the three
illumination kernels to -- with the rescale off is the colour path's restatements bit for bit, returns albedo x illumination
exactly on a one-pixel checker the colour path blurs, leaves partly covered taps and pixels and the identity tap in colour,
clamps albedos at SRT_DEMOD_EPS, and flags few pixels of the frames the GPU test renders. The entry points are exported,
declared, bound and check their arguments before they touch a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as D
import history_illumination_ref as HI
import motion_ref as M
import temporal_cases as TC
import temporal_ref as TR
import vertex_motion_ref as VM
from gpu_harness import scene
from simple_raytracer_amd import records as R, scenes as S

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
SRT_ERR_INVALID = 1
CALLS = ["srt_set_denoise_history_illumination", "srt_group_set_denoise_history_illumination", "srt_last_setup_history_illumination",
         "srt_group_last_setup_history_illumination"]
KEYS = ("h", "c", "m1", "m2", "taps", "borderline")
# the GPU test's poses: the ones of temporal_cases that start from its GENERIC pose (no whole-pixel tap coordinates)
POSES = ["dolly", "zoom_out", "roll", "big_yaw"]


def same(a, b, keys=KEYS, where=None):
    for k in keys:
        x, y = (a[k], b[k]) if where is None else (a[k][where], b[k][where])
        assert TC.same_bits(x[None], y[None]).all() if x.dtype == F32 else np.array_equal(x, y), k


# ---- the symbols ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def test_symbols_and_null_arguments(T):
    lib = T.load_library()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include/srt_abi.h").read_text(), flags=re.S)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in T.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.srt_set_denoise_history_illumination(None, 1) == SRT_ERR_INVALID
    assert lib.srt_set_denoise_history_illumination(None, 0) == SRT_ERR_INVALID
    assert lib.srt_group_set_denoise_history_illumination(None, 1) == SRT_ERR_INVALID
    assert lib.srt_last_setup_history_illumination(None) == 0 and lib.srt_group_last_setup_history_illumination(None) == 0
    for method in ("set_denoise_history_illumination", "last_setup_history_illumination"):
        assert getattr(T.TracerGroup, method) is getattr(T.Tracer, method)
    m = re.search(r"#define\s+SRT_DEMOD_EPS\s+([0-9.]+)f", code)
    assert m and F32(m.group(1)) == HI.EPS


def test_headless_history_illumination_needs_temporal(T):
    """srt_headless --history-illumination without --denoise K --temporal is a usage error, before any device is touched."""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    for args in (["--history-illumination"], ["--denoise", "5", "--history-illumination"]):
        r = subprocess.run([str(exe), "--scene", "spheres"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--history-illumination needs --denoise K --temporal" in r.stderr


# ---- the anchor: with the rescale off it is the colour path ------------------------------------------------------------------
_frames = {}


def case_frames(oracle, arrays, key, name, w, h):
    """(history frame, its record, its shape indices, current frame, its record, its shape indices) of a case of temporal_cases"""
    out = []
    for k, cam in enumerate(TC.CASES[name]):
        rdata = TC.render_record(w, h, cam, time=2000 + k)
        at = (key, w, h, rdata.tobytes())
        if at not in _frames:
            _frames[at] = TC.features_frame(oracle, rdata, *arrays)
        out += [_frames[at][0], rdata, _frames[at][1]]
    return out


def coloured_history(frame, rdata, seed=5):
    """the history a first frame commits, with a colour of its own per pixel (the oracle frames' is flat) and moments to match"""
    hist = TC.first_history(frame, rdata)
    colour = np.random.default_rng(seed).uniform(0.1, 2.0, hist["colour"].shape).astype(F32)
    m1 = D.lum(colour)
    return dict(hist, colour=colour, m1=m1, m2=(m1 * m1 + F32(0.25)).astype(F32))


@pytest.mark.parametrize("w,h", TC.SIZES)
@pytest.mark.parametrize("name", ["dolly", "zoom_out", "big_yaw"])
def test_anchor_rescale_off_is_the_colour_path(oracle, name, w, h):
    arrays = scene("mixed")
    hist_f, hist_rd, hist_ids, cur, cur_rd, ids = case_frames(oracle, arrays, "mixed", name, w, h)
    hist = coloured_history(hist_f, hist_rd)
    # without a table: srt_temporal_kernel<0, false, false>'s restatement
    off = HI.reproject(cur, hist, cur_rd, rescale=False)
    same(off, TR.reproject(cur, hist, cur_rd))
    assert not off["scaled"].any()
    # with one: a shape MOVED by a small map, the others static; the moved kernel's and the deformed kernel's restatements
    hist["ids"] = hist_ids
    n = len(arrays[0])
    moved = int(np.bincount(ids[ids < n].astype(np.int64), minlength=n).argmax())
    table = M.static_table(n)
    table["state"][moved] = M.MOVED
    table["A"][moved, 0, 3] = 0.01
    table["first_row"] = np.zeros(n, np.int64)
    none = np.zeros((0, 3, 3), F32)
    off_t = HI.reproject(cur, hist, cur_rd, ids=ids, table=table, rescale=False)
    same(off_t, TR.reproject(cur, hist, cur_rd, ids=ids, table=table), KEYS + ("state",))
    off_v = HI.reproject(cur, hist, cur_rd, ids=ids, table=table, tri_ids=np.zeros((h, w), np.uint32), rows=none, h_rows=none, rescale=False)
    same(off_v, VM.reproject(cur, hist, cur_rd, ids=ids, table=table, tri_ids=np.zeros((h, w), np.uint32), rows=none, h_rows=none), KEYS + ("state",))
    # and the rule itself changes what it should: the same taps and flags, other sums where a 2x2 straddles two materials
    # (under thresholds that let every tap with coverage count: the defaults reject most of these frames' material borders)
    loose = dict(normal_threshold=-1.0, depth_threshold=10.0)
    on, off_t = (HI.reproject(cur, hist, cur_rd, ids=ids, table=table, rescale=r, **loose) for r in (True, False))
    same(on, off_t, ("h", "taps", "borderline"))
    assert on["scaled"].any() and not TC.same_bits(on["c"], off_t["c"]).all()
    untouched = on["scaled"] == 0
    same(on, off_t, where=untouched)


# ---- the flagged share of the frames the GPU test renders ------------------------------------------------------------------
def gpu_scene(name):
    """the geometry of the GPU test's textured scenes (a texture changes no first hit)"""
    return {"noise": S.textured_noise_scene, "spheres": S.textured_sphere_scene, "mesh": S.textured_mesh_scene}[name]()[:3]


@pytest.mark.parametrize("scn", ["noise", "spheres", "mesh"])
@pytest.mark.parametrize("name", POSES)
def test_restatement_flags_under_a_thousandth_of_the_gpu_frames(oracle, scn, name):
    w, h = 128, 72
    hist_f, hist_rd, _, cur, cur_rd, _ = case_frames(oracle, gpu_scene(scn), scn, name, w, h)
    rep = HI.reproject(cur, TC.first_history(hist_f, hist_rd), cur_rd)
    flagged = int(rep["borderline"].sum())
    print(f"{scn} {name}: {flagged} of {w * h} pixels flagged, {int((rep['taps'] > 0).sum())} with taps")
    assert flagged < 1e-3 * w * h and (rep["taps"] > 0).any()


# ---- analytic: a checker plane under a translated camera -----------------------------------------------------------------------
W, H, DEPTH = 48, 32, 5.0
PIXEL = 2.0 * DEPTH / H  # world width of a pixel on the plane (fov_scale 1)


def rd(shift=0.0):
    """the camera `shift` pixel widths off the axis in x and in y (in one of them alone the other tap coordinate is a whole pixel,
    which the restatement flags)"""
    return R.render_data(W, H, 2, 10, camera_to_world=R.camera_matrix((shift * PIXEL, shift * PIXEL, DEPTH), 0.0, 0.0))


def checker(lo=0.2, hi=0.9, phase=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((xx + yy + phase) & 1)[..., None] == 0, F32(hi), F32(lo)) * np.ones(3, F32)


def plane(cam_rd, A, L, cov=None, P=2):
    """the plane z = 0 facing the camera, albedo A (h, w, 3), colour A * L: a frame of temporal_ref"""
    c0, c1, c2, cam, aspect, fov = TR.camera(cam_rd)
    ys, xs = np.mgrid[0:H, 0:W]
    sx = ((2 * (xs + 0.5) / W - 1) * float(aspect)) * float(fov)
    sy = (1 - 2 * (ys + 0.5) / H) * float(fov)
    d = np.stack([sx, sy, -np.ones_like(sx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    Z = (float(cam[2]) / -d[..., 2]).astype(F32)
    N = np.zeros((H, W, 3), F32)
    N[..., 2] = 1
    c = (np.asarray(A, F32) * np.asarray(L, F32)).astype(F32)
    m1 = D.lum(c)
    return dict(c=c, m1=m1, m2=(F32(2) * m1 * m1).astype(F32), V=np.zeros((H, W), F32), N=N, Z=Z, A=np.asarray(A, F32),
                cov=np.ones((H, W), F32) if cov is None else np.asarray(cov, F32), P=P)


def history_of(frame, cam_rd, count=6.0):
    g = np.zeros((H, W, 2, 4), F32)
    g[..., 0, :3], g[..., 0, 3] = frame["N"], frame["Z"]
    g[..., 1, :3], g[..., 1, 3] = frame["A"], frame["cov"]
    return dict(valid=True, colour=frame["c"], count=np.full((H, W), count, F32), m1=frame["m1"], m2=frame["m2"], guide=g, camera=cam_rd)


LIGHT = F32([1.3, 0.8, 0.45])


@pytest.mark.parametrize("shift", [0.5, 1.5])
def test_checker_plane_is_reprojected_as_albedo_times_light(shift):
    """history colour A_h(x) L, constant L, a one-pixel grey checker A_h; the camera translated by `shift` pixel widths in x and y, so every
    2x2 mixes both greys half and half. The rule returns A_p L at every pixel with taps for whatever A_p the frame has (here the
    checker in the other phase); the colour path returns 0.55 L. Moments follow rl and rl^2: the history's m2 is 2 m1^2."""
    hist_rd, cur_rd = rd(0.0), rd(shift)
    hist = history_of(plane(hist_rd, checker(), LIGHT), hist_rd)
    cur = plane(cur_rd, checker(phase=1), LIGHT)
    on, off = HI.reproject(cur, hist, cur_rd), HI.reproject(cur, hist, cur_rd, rescale=False)
    has = on["taps"] > 0
    assert has.sum() > 0.85 * W * H and np.array_equal(on["taps"], off["taps"]) and not on["borderline"].any()
    assert np.all(on["scaled"] == on["taps"])
    want = cur["A"] * LIGHT
    np.testing.assert_allclose(on["c"][has], want[has], rtol=1e-6, atol=0)  # a few ulp: r, the product, the weight, three sums, the quotient
    assert np.all(np.abs(off["c"][has] / want[has] - 1) > 0.1)  # the colour path: the bilinear mean of both greys
    lp = D.lum(want)
    np.testing.assert_allclose(on["m1"][has], lp[has], rtol=2e-6, atol=0)
    np.testing.assert_allclose(on["m2"][has], (2 * lp * lp)[has], rtol=3e-6, atol=0)
    assert np.array_equal(on["h"], off["h"]) and np.all(on["h"][has] == 6.0)


def test_partly_covered_taps_and_pixels_stay_in_colour():
    """coverage 0.5 on the left third of the history and on the right third of the frame: a pixel whose counted taps all come
    from there, and every pixel of the frame's third, has the colour path's bits; the middle is rescaled."""
    hist_rd, cur_rd = rd(0.0), rd(0.5)
    cov_h, cov_p = np.ones((H, W), F32), np.ones((H, W), F32)
    cov_h[:, :W // 3] = 0.5
    cov_p[:, 2 * W // 3:] = 0.5
    hist = history_of(plane(hist_rd, checker(), LIGHT, cov=cov_h), hist_rd)
    cur = plane(cur_rd, checker(phase=1), LIGHT, cov=cov_p)
    on, off = HI.reproject(cur, hist, cur_rd), HI.reproject(cur, hist, cur_rd, rescale=False)
    has = on["taps"] > 0
    xs = np.broadcast_to(np.arange(W), (H, W))
    left, right, middle = has & (xs < W // 3 - 2), has & (xs >= 2 * W // 3), has & (xs > W // 3 + 2) & (xs < 2 * W // 3)
    assert left.any() and right.any() and middle.any()
    assert not on["scaled"][left | right].any() and np.all(on["scaled"][middle] == on["taps"][middle])
    same(on, off, where=left | right)
    assert not TC.same_bits(on["c"], off["c"])[middle].any()
    mixed = has & (on["scaled"] > 0) & (on["scaled"] < on["taps"])  # a 2x2 across the history's seam: some taps rescaled, some not
    assert mixed.any()


def test_albedo_of_zero_and_nan_divides_by_eps_and_the_ratio_is_bounded():
    Ap = F32([[1.0, 0.5, 0.004], [0.0, np.nan, 1.0]])
    Ah = F32([[0.0, np.nan, 0.002], [1.0, 0.5, 0.25]])
    r, rl, both = HI.ratios(Ap, F32([1, 1]), Ah, F32([1, 1]))
    assert both.all() and np.all(np.isfinite(r)) and np.all(np.isfinite(rl))
    assert np.array_equal(r[0], F32([1.0, 0.5, 0.01]) / F32([0.01, 0.01, 0.01]))  # 0, NaN and a channel below eps: eps
    assert np.array_equal(r[1], F32([0.01, 0.01, 1.0]) / F32([1.0, 0.5, 0.25]))
    rng = np.random.default_rng(8)
    r, rl, _ = HI.ratios(rng.uniform(0, 1, (500, 3)), np.ones(500, F32), rng.uniform(0, 1, (500, 3)) * (rng.random((500, 3)) > 0.3), np.ones(500, F32))
    assert r.max() <= F32(1) / HI.EPS and rl.max() <= F32(1) / HI.EPS and r.min() >= HI.EPS
    r, rl, both = HI.ratios(Ap, F32([1, 0.5]), Ah, F32([0.75, 1]))  # a coverage below 1 on either side: no rescale
    assert not both.any() and np.all(r == 1) and np.all(rl == 1)
    # in the tap loop: a black history albedo under a white frame amplifies by 1 / eps, no more, and stays finite
    hist_rd, cur_rd = rd(0.0), rd(0.5)
    black = np.zeros((H, W, 3), F32)
    black[::2, :, 1] = np.nan
    hist = history_of(plane(hist_rd, black, LIGHT), hist_rd)
    hist["colour"] = np.full((H, W, 3), 0.02, F32)  # (what an emitter's dark texel leaves)
    on = HI.reproject(plane(cur_rd, np.ones((H, W, 3), F32), LIGHT), hist, cur_rd)
    has = on["taps"] > 0
    assert has.any() and np.all(np.isfinite(on["c"][has]))
    np.testing.assert_allclose(on["c"][has], 2.0, rtol=1e-6)


def test_a_nan_colour_tap_is_still_rejected():
    hist_rd, cur_rd = rd(0.0), rd(0.5)
    hist = history_of(plane(hist_rd, checker(), LIGHT), hist_rd)
    hist["colour"] = hist["colour"].copy()
    hist["colour"][10, 20, 1] = np.nan
    hist["colour"][11, 7, 2] = np.inf
    cur = plane(cur_rd, checker(phase=1), LIGHT)
    on, off = HI.reproject(cur, hist, cur_rd), HI.reproject(cur, hist, cur_rd, rescale=False)
    clean = HI.reproject(cur, dict(hist, colour=np.where(np.isfinite(hist["colour"]), hist["colour"], F32(1))), cur_rd)
    assert np.array_equal(on["taps"], off["taps"]) and (clean["taps"] - on["taps"]).sum() == 8  # two pixels, each a tap of four 2x2's
    assert np.all(np.isfinite(on["c"])) and np.all(np.isfinite(on["m1"])) and np.all(np.isfinite(on["m2"]))


# ---- frames that are the colour path's bit for bit ----------------------------------------------------------------------------
def test_same_camera_is_the_colour_path_bit_for_bit():
    """the identity tap is the pixel itself: not rescaled, whatever the two albedos are"""
    cam_rd = rd(0.0)
    hist = history_of(plane(cam_rd, checker(), LIGHT), cam_rd)
    cur = plane(cam_rd, checker(phase=1), LIGHT)
    on, off = HI.reproject(cur, hist, cam_rd), HI.reproject(cur, hist, cam_rd, rescale=False)
    same(on, off)
    same(on, TR.reproject(cur, hist, cam_rd))
    assert np.all(on["taps"] == 1) and not on["scaled"].any()


def test_one_albedo_everywhere_is_the_colour_path_bit_for_bit(oracle):
    """D_p and D_h bit-equal: r = x / x = 1 exactly. The sphere scene's geometry with one colour on every material, camera moved"""
    shapes, tris, mats = scene("spheres")
    mats = mats.copy()
    mats["color"][:, :3] = (0.7, 0.45, 0.3)
    w, h = 37, 29
    hist_f, hist_rd, _, cur, cur_rd, _ = case_frames(oracle, (shapes, tris, mats), "one-colour", "dolly", w, h)
    hist = coloured_history(hist_f, hist_rd)
    on, off = HI.reproject(cur, hist, cur_rd), HI.reproject(cur, hist, cur_rd, rescale=False)
    assert (on["scaled"] > 0).sum() > 0.3 * w * h
    same(on, off)
