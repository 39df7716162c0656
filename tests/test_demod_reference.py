"""CPU: albedo demodulation for the denoiser (include/srt_abi.h srt_set_denoise_demodulation). The entry points are exported,
declared, bound and check their arguments before they touch a device; the numpy restatement tests/demod_ref.py -- which
tests/test_gpu_denoise_demod.py pins the GPU filter to -- is scale invariant, beats the colour-guided filter on a one-pixel
checker, round-trips albedos below SRT_DEMOD_EPS and keeps non-finite pixels to themselves."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import demod_ref as DM
import denoise_ref as D

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
H, W = 24, 32
SRT_ERR_INVALID = 1
CALLS = ["srt_set_denoise_demodulation", "srt_group_set_denoise_demodulation", "srt_last_filter_demodulated", "srt_group_last_filter_demodulated"]


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_and_null_arguments(T):
    lib = T.load_library()
    header = (ROOT / "include/srt_abi.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in T.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    out = C.c_int(7)
    assert lib.srt_set_denoise_demodulation(None, 1) == SRT_ERR_INVALID
    assert lib.srt_set_denoise_demodulation(None, 0) == SRT_ERR_INVALID
    assert lib.srt_group_set_denoise_demodulation(None, 1) == SRT_ERR_INVALID
    assert lib.srt_last_filter_demodulated(None, C.byref(out)) == SRT_ERR_INVALID
    assert lib.srt_group_last_filter_demodulated(None, C.byref(out)) == SRT_ERR_INVALID
    assert out.value == 7
    for method in ("set_denoise_demodulation", "last_filter_demodulated"):
        assert getattr(T.TracerGroup, method) is getattr(T.Tracer, method)
    m = re.search(r"#define\s+SRT_DEMOD_EPS\s+([0-9.]+)f", code)
    assert m and F32(m.group(1)) == DM.EPS


def test_headless_demodulate_needs_denoise(T):
    """srt_headless --demodulate without --denoise K is a usage error, before any device is touched."""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    r = subprocess.run([str(exe), "--scene", "spheres", "--demodulate"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--demodulate needs --denoise" in r.stderr


# ---- synthetic set-up outputs -----------------------------------------------------------------------------------------------
def flat_guides():
    """one plane facing the camera: every tap passes the normal and depth terms"""
    N = np.broadcast_to(F32([0.0, 0.0, 1.0]), (H, W, 3)).copy()
    Z = np.full((H, W), 2.0, F32)
    cov = np.ones((H, W), F32)
    return N, Z, cov


def ramp():
    xx = np.broadcast_to(np.arange(W, dtype=np.float64) / (W - 1), (H, W))
    return np.stack([0.3 + 0.5 * xx, 0.4 + 0.3 * xx, 0.6 - 0.2 * xx], axis=-1)


def noisy_light(seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    L = ramp()
    return L, np.clip(L + rng.normal(0.0, sigma, L.shape), 0.0, None)


def test_scale_invariance():
    """One grey albedo a on every pixel: the demodulated result equals the un-demodulated denoise_ref result with the albedo
    term off. I = c / a scales colours by 1 / a and variances by 1 / a^2, and every weight depends on ratios that cancel it:
    |lp - lq| / sqrt(g(V)) (up to the 1e-10 in the denominator, far below rtol), normals and depths untouched.
    What does not cancel is float32 rounding: both sides take the luminances from float32 colours, 3e-8 of absolute error on
    values near 0.5, which the exponent multiplies by 1 / (4 sqrt(g(V))). For that to stay well under rtol = 1e-5 the
    variance must stay well above (3e-8 / 4e-5)^2 = 6e-7 through all five passes, each of which divides it by about four:
    so the input variance is 0.01 .. 0.04 (and the noise 0.15, which matches it), 1e-5 or more after the fifth pass."""
    N, Z, cov = flat_guides()
    _, c = noisy_light(3, sigma=0.15)
    c = c.astype(F32)
    V = np.random.default_rng(4).uniform(0.01, 0.04, (H, W)).astype(F32)
    for a in (0.25, 0.8):
        A = np.full((H, W, 3), a, F32)
        steps = DM.filter_steps(c, V, N, Z, A, cov, iterations=5)
        c64, V64 = c, V
        for k in range(1, 6):
            c64, V64 = D.atrous_pass(c64, V64, N, Z, A, cov, 1 << (k - 1), 4.0, 128.0, 1.0, DM.NO_ALBEDO)
            np.testing.assert_allclose(steps[k][0][..., :3], c64, rtol=1e-5, err_msg=f"a={a} K={k}")
            np.testing.assert_allclose(steps[k][0][..., 3], V64, rtol=1e-5, err_msg=f"a={a} K={k}")
    assert np.array_equal(steps[0][0][..., :3], c) and np.array_equal(steps[0][0][..., 3], V)  # K = 0: untouched


def checker_albedo(lo=(0.15, 0.2, 0.6), hi=(0.9, 0.85, 0.8)):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((xx + yy) & 1)[..., None] == 0, F32(hi), F32(lo)).astype(F32)


def test_one_pixel_checker_beats_the_guided_filter():
    """c = A * L, A a one-pixel checker, L a smooth ramp plus noise of known variance. At the default sigmas the guided
    filter's albedo term rejects the taps of the other colour; the demodulated filter averages L over all of them."""
    N, Z, cov = flat_guides()
    A = checker_albedo()
    L, Ln = noisy_light(5, sigma=0.05)
    c = (A * Ln).astype(F32)
    V = (D.lum(A) ** 2 * F32(0.05 ** 2)).astype(F32)  # the variance of lum(c), up to the channels' correlation
    truth = A * L
    guided = D.atrous_pass(c, V, N, Z, A, cov, 1, 4.0, 128.0, 1.0, 0.1)
    for k in range(1, 5):
        guided = D.atrous_pass(*guided, N, Z, A, cov, 1 << k, 4.0, 128.0, 1.0, 0.1)
    demod = DM.filter_steps(c, V, N, Z, A, cov, iterations=5)[5][0]
    mse = lambda x: float(np.mean((np.asarray(x, np.float64)[..., :3] - truth) ** 2))
    assert mse(demod) < mse(guided[0]) < mse(c)


def test_albedo_below_eps_round_trips():
    """Channels below SRT_DEMOD_EPS (0, a NaN) are divided by eps, not by themselves: nothing blows up, and a pixel that gets no
    weight from any tap returns I * D = (c / D) * D, within two roundings of c."""
    N, Z, cov = flat_guides()
    N = N.copy()
    N[5, 7] = (0.0, 1.0, 0.0)  # perpendicular to every neighbour, parallel to itself: only its own tap has weight
    A = np.full((H, W, 3), 0.5, F32)
    A[5, 7] = (0.0, 0.004, 1.0)
    A[9, 3] = (np.nan, 0.5, 0.0)
    _, c = noisy_light(6)
    c = c.astype(F32)
    c[5, 7] = (0.0, 0.003, 0.7)
    V = np.full((H, W), 0.0025, F32)
    I, VI, mask = DM.demodulate(c, V, A, cov)
    assert mask.all() and np.all(np.isfinite(I)) and np.all(I <= c / DM.EPS * (1 + 1e-6))
    assert np.array_equal(I[5, 7], c[5, 7] / F32([0.01, 0.01, 1.0]))
    o, Vo = DM.remodulate(I, VI, A, cov)
    np.testing.assert_allclose(o, c, rtol=3e-7, atol=0)
    np.testing.assert_allclose(Vo, V, rtol=5e-7, atol=0)
    hdr = DM.filter_steps(c, V, N, Z, A, cov, iterations=3)[3][0]
    np.testing.assert_allclose(hdr[5, 7, :3], c[5, 7], rtol=3e-7, atol=0)
    np.testing.assert_allclose(hdr[5, 7, 3], V[5, 7], rtol=5e-7, atol=0)
    assert np.all(np.isfinite(hdr))


def test_non_finite_pixels_neither_spread_nor_change():
    N, Z, cov = flat_guides()
    A = checker_albedo()
    _, Ln = noisy_light(7)
    c = (A * Ln).astype(F32)
    c[4, 4] = (np.nan, 0.2, 0.3)
    c[10, 20] = (0.1, np.inf, 0.3)
    cov = cov.copy()
    cov[15, 15] = 0.0  # no hits: passes through as it is, and is no tap
    V = np.full((H, W), 0.001, F32)
    steps = DM.filter_steps(c, V, N, Z, A, cov, iterations=4)
    bad = np.zeros((H, W), bool)
    bad[4, 4] = bad[10, 20] = True
    for k in range(5):
        hdr = steps[k][0]
        assert np.array_equal(hdr[bad].view(np.uint32), np.concatenate([c, V[..., None]], -1)[bad].view(np.uint32)), k
        assert np.array_equal(hdr[15, 15, :3], c[15, 15]) and hdr[15, 15, 3] == V[15, 15], k
        assert np.all(np.isfinite(hdr[~bad])), k
    # the result elsewhere is the result of a frame in which those pixels are simply not there (cov = 0)
    cov2 = cov.copy()
    cov2[bad] = 0.0
    c2 = c.copy()
    c2[bad] = 0.5
    other = DM.filter_steps(c2, V, N, Z, A, cov2, iterations=4)[4][0]
    assert np.array_equal(steps[4][0][~bad], other[~bad])
