"""numpy restatement of the denoiser's spatial variance estimate (srt_set_denoise_spatial_variance;
simple-raytracer_amd/csrc/denoise.hip srt_denoise_spatial_variance_kernel), built on tests/denoise_ref.py and
tests/demod_ref.py: a pixel with fewer than min_samples samples takes its variance from the edge-weighted means of the
moments of its 7x7 neighbourhood.

Everything is float32 in the kernel's operation order (taps dy outer, dx inner; the sums are float32 sums in that order)
except the two exponentials of a weight, which the kernel takes from the fast exp / log instructions: here they are
float64 exp / power rounded to float32, so the comparison with the GPU is within a tolerance, as for the passes.
"""
import numpy as np

import demod_ref as DM
import denoise_ref as D

F32 = np.float32
R = 3  # the window is (2 R + 1)^2 taps


def sources_spatial(canvas, moments, T, P):
    """The spatial set-up's per-pixel inputs: s = P, m1 = lum(canvas / T), m2 = M / T (float32, the set-up's expressions)."""
    canvas = np.asarray(canvas, F32)
    with np.errstate(all="ignore"):
        m1 = D.lum(canvas[..., :3] / F32(T))
        m2 = (np.asarray(moments, F32) / F32(T)).astype(F32)
    return np.full(m1.shape, F32(P), F32), m1, m2


def sources_staged(commit):
    """A temporal set-up's: the staged count and moments (temporal_ref.integrate()'s commit, or a read-back history)."""
    return np.asarray(commit["count"], F32), np.asarray(commit["m1"], F32), np.asarray(commit["m2"], F32)


def qualifies(c, cov, s, min_samples):
    """cov > 0, a finite colour and s < (float)min_samples"""
    return (np.asarray(cov) > 0) & np.all(np.isfinite(np.asarray(c, F32)), axis=-1) & (np.asarray(s, F32) < F32(min_samples))


def estimate(c, V, N, Z, A, cov, s, m1, m2, min_samples, sigma_normal=128.0, sigma_depth=1.0, sigma_albedo=0.1, demod=False, **_):
    """-> V' (h, w) float32: V with the qualifying pixels' variance replaced. c (h, w, 3) is the colour the launch sees (under
    demodulation the illumination), A the guide's albedo; demod: the moments are scaled by a = 1 / lum(max(A, eps)) and the
    albedo factor is dropped."""
    c, V, N, Z, A = (np.asarray(a, F32) for a in (c, V, N, Z, A))
    s, m1, m2 = (np.asarray(a, F32) for a in (s, m1, m2))
    h, w = V.shape
    live = (np.asarray(cov) > 0) & np.all(np.isfinite(c), axis=-1)
    ok = live & np.isfinite(m1) & np.isfinite(m2)
    q = live & (s < F32(min_samples))
    with np.errstate(all="ignore"):
        if demod:
            Dv, _ = DM.divisor(A)
            a = (F32(1) / D.lum(Dv)).astype(F32)
            m1 = (m1 * a).astype(F32)
            m2 = ((m2 * a) * a).astype(F32)
        inv_sa2 = F32(min(1.0 / (float(sigma_albedo) * float(sigma_albedo)), float(np.finfo(F32).max)))
        zs = (F32(sigma_depth) * Z).astype(F32)
        inv_dz = [(F32(1) / (zs * F32(r) + F32(1e-6))).astype(F32) for r in (1, 2, 3)]
    sw, s1, s2 = (np.zeros((h, w), F32) for _ in range(3))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            iy, ix = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            take = inside & ok[iy][:, ix]
            if dx == 0 and dy == 0:
                wgt = np.where(take, F32(1), F32(0)).astype(F32)
            else:
                Nq, Zq, Aq = N[iy][:, ix], Z[iy][:, ix], A[iy][:, ix]
                with np.errstate(all="ignore"):
                    d = ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]).astype(F32)
                    take &= d > 0
                    e = (np.abs(Z - Zq) * inv_dz[max(abs(dx), abs(dy)) - 1]).astype(F32)
                    if not demod:
                        da = A - Aq
                        e = (e + ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * inv_sa2).astype(F32)
                    wn = np.power(np.where(d > 0, d, F32(1)).astype(np.float64), float(F32(sigma_normal))).astype(F32)
                    wgt = (wn * np.exp(-e.astype(np.float64)).astype(F32)).astype(F32)
                wgt = np.where(take, wgt, F32(0)).astype(F32)
            with np.errstate(all="ignore"):
                sw = np.where(take, sw + wgt, sw).astype(F32)
                s1 = np.where(take, s1 + wgt * m1[iy][:, ix], s1).astype(F32)
                s2 = np.where(take, s2 + wgt * m2[iy][:, ix], s2).astype(F32)
    with np.errstate(all="ignore"):
        p1, p2 = (s1 / sw).astype(F32), (s2 / sw).astype(F32)
        v = (p2 - p1 * p1).astype(F32)
        v = (np.where(v > F32(0), v, F32(0)).astype(F32) / s).astype(F32)
        v = np.where(np.isfinite(v), v, F32(0)).astype(F32)
    return np.where(q, v, V).astype(F32)


def filter_steps(c, V, N, Z, A, cov, s, m1, m2, min_samples, iterations=5, demod=False, **sigmas):
    """The filter over a set-up's output (denoise_ref.setup's, or temporal_ref.temporal_setup's c, V and its cur N, Z, A,
    cov) with the estimate between the set-up and the passes, for K = 0 .. iterations: a list of (hdr (h, w, 4) float32,
    argb (h, w, 4) uint8), and the {colour, variance} right after the estimate's launch (under demodulation {I, V_I}) as
    (h, w, 4) float32. K = 0: the set-up's own image. min_samples = 0: denoise_ref's / demod_ref's steps."""
    c, V = np.asarray(c, F32), np.asarray(V, F32)
    out = [(np.concatenate([c, V[..., None]], axis=-1), D.tonemap(c))]
    sig = {k: sigmas.get(k, D.DEFAULTS[k]) for k in ("sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo")}
    x, Vx = c, V
    if demod:
        x, Vx, _ = DM.demodulate(c, V, A, cov)
    if min_samples:
        Vx = estimate(x, Vx, N, Z, A, cov, s, m1, m2, min_samples, demod=demod, **sig)
    after = np.concatenate([x, Vx[..., None]], axis=-1).astype(F32)
    x64, V64 = x, Vx
    Af = np.where(np.isfinite(A), A, F32(0)) if demod else A
    for i in range(1, iterations + 1):
        if demod:
            x64, V64 = D.atrous_pass(x64, V64, N, Z, Af, cov, 1 << (i - 1), sig["sigma_luminance"], sig["sigma_normal"], sig["sigma_depth"], DM.NO_ALBEDO)
            o, Vo = DM.remodulate(x64, V64, Af, cov)
        else:
            x64, V64 = D.atrous_pass(x64, V64, N, Z, A, cov, 1 << (i - 1), **sig)
            o, Vo = np.asarray(x64, F32), np.asarray(V64, F32)
        out.append((np.concatenate([o, Vo[..., None]], axis=-1), D.tonemap(o)))
    return out, after
