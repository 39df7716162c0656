"""The numpy restatement of the spatial variance estimate (tests/spatial_variance_ref.py) on its own: what it leaves alone,
what pooling equal values gives, that pooling beats the per-pixel estimate on two-sample moments, edges, borders and the
demodulated form. No GPU."""
import numpy as np
import pytest

import demod_ref as DM
import denoise_ref as D
import spatial_variance_ref as SV

F32 = np.float32


def flat(h, w, normal=(0.0, 0.0, 1.0), z=5.0, albedo=(0.5, 0.5, 0.5)):
    """a flat region: c, V, N, Z, A, cov"""
    c = np.full((h, w, 3), 0.25, F32)
    V = np.full((h, w), 0.125, F32)
    N = np.broadcast_to(np.asarray(normal, F32), (h, w, 3)).copy()
    Z = np.full((h, w), z, F32)
    A = np.broadcast_to(np.asarray(albedo, F32), (h, w, 3)).copy()
    cov = np.ones((h, w), F32)
    return c, V, N, Z, A, cov


def two_sample_moments(rng, h, w, mean=1.0, sd=0.5):
    """per-pixel moments of two i.i.d. samples: m1, m2, and the per-pixel estimate max(0, m2 - m1^2) / 2"""
    x = rng.normal(mean, sd, (h, w, 2)).astype(F32)
    m1 = ((x[..., 0] + x[..., 1]) / F32(2)).astype(F32)
    m2 = ((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) / F32(2)).astype(F32)
    v = m2 - m1 * m1
    return m1, m2, (np.where(v > 0, v, F32(0)) / F32(2)).astype(F32)


def direct(N, Z, A, ok, m1, m2, s, x, y, sn=128.0, sz=1.0, sa=0.1, albedo=True):
    """the estimate of pixel (x, y) by a double loop over its clipped window, in float64"""
    h, w = Z.shape
    sw = s1 = s2 = 0.0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            qx, qy = x + dx, y + dy
            if not (0 <= qx < w and 0 <= qy < h) or not ok[qy, qx]:
                continue
            if dx == 0 and dy == 0:
                wgt = 1.0
            else:
                d = float(np.dot(N[y, x].astype(np.float64), N[qy, qx].astype(np.float64)))
                if d <= 0:
                    continue
                r = max(abs(dx), abs(dy))
                wgt = d ** sn * np.exp(-abs(float(Z[y, x]) - float(Z[qy, qx])) / (sz * float(Z[y, x]) * r + 1e-6))
                if albedo:
                    wgt *= np.exp(-float(np.sum((A[y, x].astype(np.float64) - A[qy, qx]) ** 2)) / (sa * sa))
            sw += wgt
            s1 += wgt * float(m1[qy, qx])
            s2 += wgt * float(m2[qy, qx])
    if sw == 0:
        return 0.0
    v = max(0.0, s2 / sw - (s1 / sw) ** 2) / float(s)
    return v if np.isfinite(v) else 0.0


# ---- 1. nothing qualifies -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [0, 1, 2])
def test_enough_samples_everywhere_is_identity(min_samples):
    rng = np.random.default_rng(1)
    c, V, N, Z, A, cov = flat(9, 11)
    V = rng.random((9, 11)).astype(F32)
    m1, m2, _ = two_sample_moments(rng, 9, 11)
    s = np.full((9, 11), 2, F32)
    out = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, min_samples)
    assert np.array_equal(out.view(np.uint32), V.view(np.uint32))
    s[4, 5] = 1  # one pixel below min_samples = 2: it alone changes
    out = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 2)
    changed = out.view(np.uint32) != V.view(np.uint32)
    assert changed[4, 5] and changed.sum() == 1


# ---- 2. pooling equal values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, 2.0, 7.0])
def test_constant_moments_give_the_per_pixel_formula(s):
    c, V, N, Z, A, cov = flat(12, 10)
    m1 = np.full((12, 10), 0.75, F32)
    m2 = np.full((12, 10), 1.5, F32)
    out = SV.estimate(c, V, N, Z, A, cov, np.full((12, 10), s, F32), m1, m2, 8)
    want = max(0.0, 1.5 - 0.75 * 0.75) / s
    np.testing.assert_allclose(out, want, rtol=1e-6)


# ---- 3. pooled against per-pixel on two-sample moments -------------------------------------------------------------------
def test_pooled_estimate_beats_the_per_pixel_one():
    rng = np.random.default_rng(20171)
    h, w, sd = 29, 33, 0.5
    c, V, N, Z, A, cov = flat(h, w)
    m1, m2, per_pixel = two_sample_moments(rng, h, w, sd=sd)
    # a tenth of the pixels: two samples that agree, so the per-pixel estimate is exactly 0 there
    same = rng.random((h, w)) < 0.1
    m2 = np.where(same, m1 * m1, m2).astype(F32)
    per_pixel = np.where(same, F32(0), per_pixel)
    pooled = SV.estimate(c, per_pixel, N, Z, A, cov, np.full((h, w), 2, F32), m1, m2, 8)
    true = sd * sd / 2  # the variance of the mean of two samples
    err_pixel = float(np.mean(np.abs(per_pixel - true)))
    err_pooled = float(np.mean(np.abs(pooled - true)))
    print(f"mean |V - true|: per pixel {err_pixel:.4f}, pooled {err_pooled:.4f}; V == 0: {np.mean(per_pixel == 0):.3f} / {np.mean(pooled == 0):.3f}")
    assert err_pooled < err_pixel
    assert np.mean(pooled == 0) < np.mean(per_pixel == 0)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
def test_taps_that_do_not_count_contribute_nothing():
    rng = np.random.default_rng(3)
    h, w = 7, 7
    c, V, N, Z, A, cov = flat(h, w)
    m1, m2, _ = two_sample_moments(rng, h, w)
    s = np.full((h, w), 2, F32)
    base = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 8)
    # poison four taps of the centre pixel's window in four ways, and give them absurd moments
    N2, cov2, c2, m1b, m2b = N.copy(), cov.copy(), c.copy(), m1.copy(), m2.copy()
    N2[1, 1] = (1.0, 0.0, 0.0)  # across a normal edge: N.Nq = 0
    cov2[2, 5] = 0.0
    c2[5, 2, 1] = np.nan
    m1b[[1, 2, 5], [1, 5, 2]] = 1e6
    m2b[[1, 2, 5], [1, 5, 2]] = 1e12
    m1b[5, 5], m2b[4, 1] = np.nan, np.inf
    bad = np.zeros((h, w), bool)
    bad[[1, 2, 5, 5, 4], [1, 5, 2, 5, 1]] = True
    got = SV.estimate(c2, V, N2, Z, A, cov2, s, m1b, m2b, 8)
    want = direct(N2, Z, A, ~bad, m1, m2, 2, 3, 3)
    np.testing.assert_allclose(got[3, 3], want, rtol=1e-5)
    assert np.isfinite(got).all()
    # and the same number when the poisoned taps are simply absent
    ok = ~bad
    m1c, m2c = np.where(ok, m1, np.nan).astype(F32), np.where(ok, m2, np.nan).astype(F32)
    np.testing.assert_allclose(SV.estimate(c, V, N, Z, A, cov, s, m1c, m2c, 8)[3, 3], got[3, 3], rtol=1e-6)
    assert base[3, 3] != got[3, 3]


def test_half_planes_keep_their_own_side():
    h, w = 10, 14
    c, V, N, Z, A, cov = flat(h, w)
    N[:, 7:] = (1.0, 0.0, 0.0)  # perpendicular to the left half's (0, 0, 1)
    m1 = np.where(np.arange(w)[None, :] < 7, F32(1.0), F32(3.0)) * np.ones((h, 1), F32)
    m2 = np.where(np.arange(w)[None, :] < 7, F32(1.5), F32(13.0)) * np.ones((h, 1), F32)
    out = SV.estimate(c, V, N, Z, A, cov, np.full((h, w), 2, F32), m1.astype(F32), m2.astype(F32), 8)
    np.testing.assert_allclose(out[:, :7], (1.5 - 1.0) / 2, rtol=1e-6)
    np.testing.assert_allclose(out[:, 7:], (13.0 - 9.0) / 2, rtol=1e-6)


# ---- 5. borders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (7, 7)])
def test_small_frames_against_a_double_loop(w, h):
    rng = np.random.default_rng(100 * w + h)
    c, V, N, Z, A, cov = flat(h, w)
    Z = (5.0 + rng.random((h, w))).astype(F32)
    A = (0.5 + 0.05 * rng.random((h, w, 3))).astype(F32)
    n = rng.normal(0, 0.05, (h, w, 3)) + (0, 0, 1)
    N = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    m1, m2, _ = two_sample_moments(rng, h, w)
    out = SV.estimate(c, V, N, Z, A, cov, np.full((h, w), 2, F32), m1, m2, 8)
    assert np.isfinite(out).all()
    ok = np.ones((h, w), bool)
    for y in range(h):
        for x in range(w):
            np.testing.assert_allclose(out[y, x], direct(N, Z, A, ok, m1, m2, 2, x, y), rtol=2e-4, atol=1e-7)


# ---- 6. the demodulated form ---------------------------------------------------------------------------------------------
def test_demodulated_constant_albedo_scales_the_colour_space_result():
    rng = np.random.default_rng(6)
    h, w = 9, 13
    albedo = (0.6, 0.3, 0.2)
    c, V, N, Z, A, cov = flat(h, w, albedo=albedo)
    m1, m2, _ = two_sample_moments(rng, h, w)
    s = np.full((h, w), 2, F32)
    colour = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 8)
    illum = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 8, demod=True)
    l = float(D.lum(np.maximum(np.asarray(albedo, F32), DM.EPS)))
    np.testing.assert_allclose(illum, colour / (l * l), rtol=1e-5)


def test_demodulated_checker_albedo_drops_the_albedo_factor():
    h, w = 10, 12
    c, V, N, Z, A, cov = flat(h, w)
    checker = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)
    A[checker] = (0.9, 0.8, 0.1)
    A[~checker] = (0.1, 0.2, 0.7)
    lD = D.lum(np.maximum(A, DM.EPS))
    i1, i2 = F32(2.0), F32(5.0)  # constant illumination moments; the colour-space ones carry the albedo's luminance
    m1 = (i1 * lD).astype(F32)
    m2 = (i2 * lD * lD).astype(F32)
    s = np.full((h, w), 2, F32)
    illum = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 8, demod=True)
    np.testing.assert_allclose(illum, (5.0 - 4.0) / 2, rtol=1e-4)
    # with the albedo factor (the colour form, sigma_albedo = 0.1) the two colours would not pool: each pixel sees only its own
    colour = SV.estimate(c, V, N, Z, A, cov, s, m1, m2, 8)
    np.testing.assert_allclose(colour, np.maximum(m2 - m1 * m1, 0) / 2, rtol=1e-4)


def test_filter_steps_without_the_switch_are_the_existing_references():
    rng = np.random.default_rng(9)
    h, w = 8, 9
    c, V, N, Z, A, cov = flat(h, w)
    c = rng.random((h, w, 3)).astype(F32)
    V = rng.random((h, w)).astype(F32)
    m1, m2, _ = two_sample_moments(rng, h, w)
    s = np.full((h, w), 2, F32)
    steps, _ = SV.filter_steps(c, V, N, Z, A, cov, s, m1, m2, 0, iterations=2)
    want = DM.filter_steps(c, V, N, Z, A, cov, iterations=2)
    steps_d, _ = SV.filter_steps(c, V, N, Z, A, cov, s, m1, m2, 0, iterations=2, demod=True)
    for k in range(3):
        assert np.array_equal(steps_d[k][0].view(np.uint32), want[k][0].view(np.uint32)), k
    c64, V64 = c, V
    for k in range(1, 3):
        c64, V64 = D.atrous_pass(c64, V64, N, Z, A, cov, 1 << (k - 1), **{kk: D.DEFAULTS[kk] for kk in D.DEFAULTS if kk != "iterations"})
        assert np.array_equal(steps[k][0][..., :3].view(np.uint32), np.asarray(c64, F32).view(np.uint32)), k
