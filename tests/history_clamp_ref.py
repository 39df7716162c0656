"""The history clamp (include/srt_abi.h srt_set_denoise_history_clamp; simple-raytracer_amd/csrc/temporal.hip
srt_temporal_bounds_kernel and srt_temporal_kernel with CLAMP true) in numpy, on top of
tests/history_illumination_ref.py's reprojection (the superset of the set-up kernels) and tests/temporal_ref.py's integration.

    bounds   per pixel p with cov > 0 and a finite colour, over its 7x7 taps q (dy outer, dx inner) that are inside the image,
             have cov > 0 and a finite colour: the centre weighs 1, another tap the spatial variance estimate's geometric weight
             (tests/spatial_variance_ref.py: depth term with r = max(|dx|, |dy|), normal power, albedo term; Np.Nq <= 0: 0).
             mu = sum w c / sum w, s = sum w (c c) / sum w, sigma = sqrt(max(0, s - mu mu)) per channel, evaluated as the kernel
             does on e = c_q - c_p: d = sum w e / sum w, q = sum w (e e) / sum w, mu = c_p + d, sigma = sqrt(max(0, q - d d)).
             weight = sum w, stored as 0 ("do not clamp") with fewer than 5 counting taps or a mu or q that is not finite.
    clamp    the reprojected history colour x of a pixel with weight > 0, per channel: x < mu - gamma sigma -> that bound, else
             x > mu + gamma sigma -> that bound. A channel moved: m1' = lum(x'), m2' = max(0, m2 - m1 m1) + m1' m1'.

Everything float32 in the kernel's order, unfused, except a weight's two exponentials, which the kernel takes from the fast
exp / log instructions (float64 here, rounded): the planes agree with the device within a tolerance, the tap counts exactly.
A pixel whose history colour lies within rtol 1e-4 of a bound it is compared with is flagged `borderline`: device and numpy
may decide it either way.
"""
import numpy as np

import denoise_ref as D
import history_illumination_ref as HI
import temporal_ref as TR

F32 = np.float32
R = 3
MIN_TAPS = 5


def bounds(cur, sigma_normal=128.0, sigma_depth=1.0, sigma_albedo=0.1, **_):
    """cur: temporal_ref.frame()'s dict (c, N, Z, A, cov) -> dict mu (h, w, 3), weight (h, w), sigma (h, w, 3), taps (h, w)
    int32, sum_w (h, w): the sum of weights before the two "do not clamp" rules."""
    c, N, Z, A = (np.asarray(cur[k], F32) for k in ("c", "N", "Z", "A"))
    h, w = Z.shape
    ok = (np.asarray(cur["cov"]) > 0) & np.all(np.isfinite(c), axis=-1)
    with np.errstate(all="ignore"):
        inv_sa2 = F32(min(1.0 / (float(sigma_albedo) * float(sigma_albedo)), float(np.finfo(F32).max)))
        zs = (F32(sigma_depth) * Z).astype(F32)
        inv_dz = [(F32(1) / (zs * F32(r) + F32(1e-6))).astype(F32) for r in (1, 2, 3)]
    sw = np.zeros((h, w), F32)
    s1, s2 = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
    taps = np.zeros((h, w), np.int32)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            iy, ix = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            counts = ok & inside & ok[iy][:, ix]
            taps += counts
            with np.errstate(all="ignore"):
                cq = (c[iy][:, ix] - c).astype(F32)
            if dx == 0 and dy == 0:
                take, wgt = counts, np.ones((h, w), F32)
            else:
                Nq, Zq, Aq = N[iy][:, ix], Z[iy][:, ix], A[iy][:, ix]
                with np.errstate(all="ignore"):
                    d = ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]).astype(F32)
                    take = counts & (d > 0)
                    da = A - Aq
                    e = (np.abs(Z - Zq) * inv_dz[max(abs(dx), abs(dy)) - 1]
                         + ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * inv_sa2).astype(F32)
                    wn = np.power(np.where(d > 0, d, F32(1)).astype(np.float64), float(F32(sigma_normal))).astype(F32)
                    wgt = (wn * np.exp(-e.astype(np.float64)).astype(F32)).astype(F32)
            with np.errstate(all="ignore"):
                sw = np.where(take, sw + wgt, sw).astype(F32)
                s1 = np.where(take[..., None], s1 + wgt[..., None] * cq, s1).astype(F32)
                s2 = np.where(take[..., None], s2 + wgt[..., None] * (cq * cq), s2).astype(F32)
    with np.errstate(all="ignore"):
        one = np.where(ok, sw, F32(1))[..., None]
        d, s = (s1 / one).astype(F32), (s2 / one).astype(F32)
        mu = (c + d).astype(F32)
        var = (s - d * d).astype(F32)
        sigma = np.sqrt(np.where(var > F32(0), var, F32(0)).astype(F32)).astype(F32)
    use = ok & (taps >= MIN_TAPS) & np.all(np.isfinite(mu), axis=-1) & np.all(np.isfinite(s), axis=-1)
    z3 = np.zeros((h, w, 3), F32)
    return dict(mu=np.where(ok[..., None], mu, z3), weight=np.where(use, sw, F32(0)).astype(F32), sigma=np.where(ok[..., None], sigma, z3),
                taps=np.where(ok, taps, 0).astype(np.int32), sum_w=np.where(ok, sw, F32(0)).astype(F32))


def clamp(rep, b, gamma):
    """rep: a reprojection (temporal_ref.reproject's dict: h, c, m1, m2, ...), b: bounds() -> a copy of rep with the colour and
    moments clamped, 'clamped' (h, w) bool: a channel moved on a pixel that has history, and 'near_edge' (h, w) bool: the
    history colour lies within rtol 1e-4 of a bound."""
    g = F32(gamma)
    x, m1, m2 = (np.asarray(rep[k], F32) for k in ("c", "m1", "m2"))
    on = (np.asarray(rep["h"], F32) > 0) & (b["weight"] > 0)
    with np.errstate(all="ignore"):
        e = (g * b["sigma"]).astype(F32)
        lo, hi = (b["mu"] - e).astype(F32), (b["mu"] + e).astype(F32)
        below, above = x < lo, ~(x < lo) & (x > hi)
        y = np.where(below, lo, np.where(above, hi, x)).astype(F32)
        moved = on & (below | above).any(-1)
        near = on & (np.isclose(x, lo, rtol=1e-4, atol=0) | np.isclose(x, hi, rtol=1e-4, atol=0)).any(-1)
        var = (m2 - m1 * m1).astype(F32)
        var = np.where(var > F32(0), var, F32(0)).astype(F32)
        n1 = D.lum(y)
        n2 = (var + n1 * n1).astype(F32)
    out = dict(rep)
    out["c"] = np.where(moved[..., None], y, x).astype(F32)
    out["m1"] = np.where(moved, n1, m1).astype(F32)
    out["m2"] = np.where(moved, n2, m2).astype(F32)
    out["clamped"], out["near_edge"] = moved, near
    return out


def temporal_setup(canvas, inputs, F, hist, cam_rd, gamma, history_limit=32, normal_threshold=0.9, depth_threshold=0.05, ids=None, table=None,
                   tri_ids=None, rows=None, h_rows=None, rescale=False, sigmas=None):
    """The whole set-up with the clamp (history_illumination_ref.temporal_setup's arguments; rescale: the history illumination
    switch; sigmas: the filter's, for the weights). -> temporal_ref.integrate()'s dict with the clamped reprojection under
    'rep' (its 'borderline' also holds the pixels near a bound), the unclamped one under 'rep_off', 'cur', 'bounds', and
    'off': the set-up without the clamp. gamma 0, or no history: the clamp does not run ('bounds' None)."""
    cur = TR.frame(canvas, inputs, F)
    if not (table is not None and hist["valid"] and np.any(table["state"] != TR.STATIC)):
        ids = table = None
    if table is None or not np.any(table["state"] == HI.DEFORMED):
        tri_ids = rows = h_rows = None
    rep = HI.reproject(cur, hist, cam_rd, normal_threshold, depth_threshold, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows,
                       rescale=rescale)
    off = TR.integrate(cur, rep, history_limit)
    b = None
    used = rep
    if gamma and hist["valid"]:
        b = bounds(cur, **(sigmas or {}))
        used = clamp(rep, b, gamma)
        used["borderline"] = rep["borderline"] | used["near_edge"]
    else:
        used = dict(rep, clamped=np.zeros(cur["Z"].shape, bool), near_edge=np.zeros(cur["Z"].shape, bool))
    out = TR.integrate(cur, used, history_limit)
    out["rep"], out["rep_off"], out["cur"], out["bounds"], out["off"] = used, rep, cur, b, off
    return out
