"""CPU: the history feedback's restatement (tests/feedback_ref.py; include/srt_abi.h srt_set_denoise_history_feedback) on analytic
inputs, the symbols and their NULL arguments, and srt_headless's usage rule."""
import re
from pathlib import Path

import numpy as np
import pytest

import demod_ref as DM
import denoise_ref as D
import feedback_ref as FB
import temporal_ref as TR
from conftest import bits_equal

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
SRT_ERR_INVALID = 1
CALLS = ["srt_set_denoise_history_feedback", "srt_group_set_denoise_history_feedback", "srt_last_filter_history_feedback",
         "srt_group_last_filter_history_feedback"]
W, H = 12, 9
HK = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
FLAT_LUM = dict(sigma_luminance=1e30)  # the luminance term vanishes: the weights are the spatial kernel's alone


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
    for e in (0, 1):
        assert lib.srt_set_denoise_history_feedback(None, e) == SRT_ERR_INVALID
        assert lib.srt_group_set_denoise_history_feedback(None, e) == SRT_ERR_INVALID
    assert lib.srt_last_filter_history_feedback(None) == 0 and lib.srt_group_last_filter_history_feedback(None) == 0
    for method in ("set_denoise_history_feedback", "last_filter_history_feedback"):
        assert getattr(T.TracerGroup, method) is getattr(T.Tracer, method)


def test_headless_history_feedback_needs_temporal(T):
    """srt_headless --history-feedback without --denoise K --temporal is a usage error, before any device is touched"""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    for args in (["--history-feedback"], ["--denoise", "5", "--history-feedback"]):
        r = subprocess.run([str(exe), "--scene", "spheres"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--history-feedback needs --denoise K --temporal" in r.stderr


# ---- analytic set-ups ------------------------------------------------------------------------------------------------------------
def wall(c, A=0.5, V=1.0):
    """a set-up's dict (temporal_ref.integrate's layout) over a wall facing the camera at depth 5: colour c (H, W, 3), albedo A
    (a number or (H, W, 3)), variance V everywhere, full coverage, six samples of history"""
    c = np.asarray(c, F32)
    N = np.zeros((H, W, 3), F32)
    N[..., 2] = 1
    cur = dict(c=c, N=N, Z=np.full((H, W), F32(5)), A=(np.ones((H, W, 3), F32) * np.asarray(A, F32)).astype(F32), cov=np.ones((H, W), F32), P=2)
    guide = np.zeros((H, W, 2, 4), F32)
    guide[..., 0, :3], guide[..., 0, 3], guide[..., 1, :3], guide[..., 1, 3] = cur["N"], cur["Z"], cur["A"], cur["cov"]
    m1 = D.lum(np.where(np.isfinite(c), c, F32(0)))
    commit = dict(colour=c.copy(), count=np.full((H, W), F32(6)), m1=m1, m2=(m1 * m1 + F32(1)).astype(F32), guide=guide)
    return dict(c=c, V=np.full((H, W), F32(V)), cur=cur, commit=commit)


def unchanged_but_colour(got, st):
    for k in ("count", "m1", "m2", "guide"):
        assert bits_equal(got[k], st["commit"][k]), k


def test_a_constant_image_comes_back_unchanged():
    st = wall(np.ones((H, W, 3), F32) * F32((0.5, 0.25, 0.75)))
    for demod in (False, True):
        got = FB.feed_back(st, 5, demod=demod)
        assert got["written"].all()
        assert bits_equal(got["colour"], st["c"]), demod
        unchanged_but_colour(got, st)


@pytest.mark.parametrize("where", [(4, 6), (0, 5), (4, 0), (0, 0), (H - 1, W - 1)], ids=["interior", "top edge", "left edge", "corner", "far corner"])
def test_an_impulse_becomes_the_binomial_pattern(where):
    """with the luminance term gone every in-image tap of pixel p has weight h(dx) h(dy): p's result is the impulse times its
    tap's weight over the sum of p's in-image weights -- the 5x5 h (x) h around the impulse, renormalised at the borders"""
    iy, ix = where
    c = np.zeros((H, W, 3), F32)
    c[iy, ix] = (2.0, 1.0, 0.5)
    got = FB.feed_back(wall(c), 1, **FLAT_LUM)
    want = np.zeros((H, W, 3))
    for py in range(H):
        for px in range(W):
            norm = sum(HK[dy + 2] * HK[dx + 2] for dy in range(-2, 3) for dx in range(-2, 3) if 0 <= py + dy < H and 0 <= px + dx < W)
            if abs(iy - py) <= 2 and abs(ix - px) <= 2:
                want[py, px] = c[iy, ix].astype(np.float64) * HK[iy - py + 2] * HK[ix - px + 2] / norm
    assert got["written"].all()
    np.testing.assert_allclose(got["colour"], want, rtol=1e-6, atol=0)  # float32 rounding of a float64 sum
    assert got["colour"][iy, ix, 0] < 2.0 * 0.15 / (1.0 if where == (4, 6) else 0.3)  # (9/64 of the impulse inside; more at a border, never all)
    interior = (got["colour"][2:-2, 2:-2].sum((0, 1)), c[iy, ix]) if where == (4, 6) else None
    if interior:
        np.testing.assert_allclose(*interior, rtol=1e-6)  # inside, the pattern sums to the impulse


def test_pixels_that_are_no_centre_are_no_tap_and_keep_their_colour():
    c = np.ones((H, W, 3), F32) * F32(0.5)
    c[3, 3] = 7.0            # sky: cov = 0
    c[5, 8, 1] = np.nan      # a non-finite colour
    c[6, 2] = np.inf
    st = wall(c)
    st["cur"]["cov"][3, 3] = 0
    st["cur"]["N"][3, 3] = 0
    st["commit"]["guide"][3, 3] = 0
    for demod in (False, True):
        got = FB.feed_back(st, 2, demod=demod, **FLAT_LUM)
        skipped = np.zeros((H, W), bool)
        skipped[3, 3] = skipped[5, 8] = skipped[6, 2] = True
        assert np.array_equal(got["written"], ~skipped)
        assert bits_equal(got["colour"][skipped], c[skipped])  # the set-up's colour, bit for bit
        assert bits_equal(got["colour"][~skipped], c[~skipped])  # and none of 7, NaN or inf reached a neighbour: still 0.5
        unchanged_but_colour(got, st)


def test_a_pixel_without_weight_keeps_its_colour():
    """a centre whose normal is zero has no tap with N.N > 0, not even itself"""
    c = (np.arange(H * W * 3, dtype=F32).reshape(H, W, 3) / F32(7)).astype(F32)
    st = wall(c)
    st["cur"]["N"][4, 4] = 0
    for demod in (False, True):
        got = FB.feed_back(st, 3, demod=demod)
        assert not got["written"][4, 4] and got["written"].sum() == H * W - 1
        assert bits_equal(got["colour"][4, 4], c[4, 4])


def test_demodulation_feeds_back_colour_not_illumination():
    """a two-albedo checker under constant illumination (numbers whose quotients are exact): in the demodulated space pass 1 sees
    a constant and returns it bit for bit, and what goes back is I D = the colour; without demodulation (and an albedo term too wide
    to separate the two) the same pass blurs the checker"""
    yy, xx = np.mgrid[:H, :W]
    A = np.where(((yy + xx) & 1)[..., None] == 0, F32(0.5), F32(0.25)) * np.ones(3, F32)
    illum = F32(1.5)
    c = (A * illum).astype(F32)
    st = wall(c, A=A)
    I, _, mask = DM.demodulate(st["c"], st["V"], A, st["cur"]["cov"])
    assert mask.all() and np.all(I == illum)
    got = FB.feed_back(st, 5, demod=True)
    assert got["written"].all()
    assert bits_equal(got["colour"], (I * DM.divisor(A)[0]).astype(F32)) and bits_equal(got["colour"], c)
    blurred = FB.feed_back(st, 5, demod=False, sigma_albedo=1e3, **FLAT_LUM)
    assert np.abs(blurred["colour"] - c).max() > 0.1
    # K = 1: the pass is the last one, its remodulated output is the value -- the same expression
    assert bits_equal(FB.feed_back(st, 1, demod=True)["colour"], got["colour"])
    # an albedo below SRT_DEMOD_EPS divides and multiplies by eps
    dark = wall((np.ones((H, W, 3)) * 0.004).astype(F32), A=0.001)
    got = FB.feed_back(dark, 1, demod=True)
    np.testing.assert_allclose(got["colour"], dark["c"], rtol=1e-6)


def test_no_pass_no_feedback():
    rng = np.random.default_rng(5)
    st = wall(rng.random((H, W, 3)).astype(F32))
    for demod in (False, True):
        got = FB.feed_back(st, 0, demod=demod, min_samples=8)
        assert not got["written"].any()
        for k in ("colour", "count", "m1", "m2", "guide"):
            assert bits_equal(got[k], st["commit"][k]), k
    assert not bits_equal(FB.feed_back(st, 1)["colour"], st["commit"]["colour"])


def test_the_spatial_variance_estimate_comes_before_the_pass():
    """few samples everywhere (count 6 < 8): the estimate replaces the variance pass 1 weighs luminance with, so the colour fed
    back differs from the one without it; count and moments are read, never written"""
    rng = np.random.default_rng(6)
    st = wall(rng.random((H, W, 3)).astype(F32), V=1e-4)
    a, b = FB.feed_back(st, 5, min_samples=0), FB.feed_back(st, 5, min_samples=8)
    assert not bits_equal(a["colour"], b["colour"])
    unchanged_but_colour(b, st)


def test_whole_setup_from_a_frame():
    """temporal_setup over a synthetic frame without a history: the set-up is the spatial one, and the feedback set is feed_back's"""
    rng = np.random.default_rng(7)
    canvas = np.zeros((H, W, 4), F32)
    canvas[..., :3] = rng.random((H, W, 3)) * 2
    nd = np.zeros((H, W, 4), F32)
    nd[..., 2], nd[..., 3] = 1, 5
    ah = np.ones((H, W, 4), F32) * F32((0.5, 0.5, 0.5, 1))
    inputs = dict(normal_depth=nd, albedo_hits=ah, moments=(D.lum(canvas[..., :3]) ** 2 * 2).astype(F32), T=1, P=2)
    hist = dict(valid=False, colour=np.zeros((H, W, 3), F32), count=np.zeros((H, W), F32), m1=np.zeros((H, W), F32), m2=np.zeros((H, W), F32),
                guide=np.zeros((H, W, 2, 4), F32), camera=None)
    from simple_raytracer_amd import records as R, scenes as S
    rd = R.render_data(W, H, 2, 10, camera_to_world=S.default_camera(), time=1)
    out = FB.temporal_setup(canvas, inputs, 1, hist, rd, iterations=5)
    plain = TR.temporal_setup(canvas, inputs, 1, hist, rd)
    for k in ("count", "m1", "m2", "guide"):
        assert bits_equal(out["commit_fb"][k], plain["commit"][k]), k
    assert bits_equal(out["commit"]["colour"], plain["commit"]["colour"])
    assert out["commit_fb"]["written"].all() and not bits_equal(out["commit_fb"]["colour"], plain["commit"]["colour"])
