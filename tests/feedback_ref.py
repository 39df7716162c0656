"""The history feedback (include/srt_abi.h srt_set_denoise_history_feedback) restated in numpy from the pieces the other
restatements already are: the temporal set-up (history_clamp_ref.temporal_setup, which is temporal_ref's with history
illumination and the clamp as options), demod_ref's demodulate and divisor, spatial_variance_ref's estimate and
denoise_ref.atrous_pass. Nothing of them is restated here.

With the switch on and K >= 1 passes, pass 1 (step 1; after the demodulate step and the spatial variance estimate where those
are on) also writes its colour result into the staged colour: for a pixel that entered the filter branch (cov > 0 and a finite
input), received weight and whose three values are finite. Under demodulation the value is I' D_p in float32. Every other
pixel keeps the set-up's colour bit for bit; count, moments and guide are never touched. K = 0: the set-up's staging set.

denoise_ref.atrous_pass returns a pixel that got no weight unchanged and does not say which those are. `written` therefore is:
the pass changed the pixel, or its own centre tap counts (N.N > 0 and a finite exponent: the centre's weight is then
h(0)^2 > 0). A pixel whose sum a NaN-weighted neighbour poisoned is unfiltered on the device and may be judged written here; its
two candidates are c and (c / D) D, equal within float32 rounding, far inside the tolerance of a pass against numpy."""
import numpy as np

import demod_ref as DM
import denoise_ref as D
import history_clamp_ref as HC
import spatial_variance_ref as SV

F32 = np.float32
SIGMAS = ("sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo")


def pass1_colour(c, V, N, Z, A, cov, src=None, demod=False, min_samples=0, **sigmas):
    """Pass 1 over a set-up's output c (h, w, 3), V (h, w) with the guide N, Z, A, cov. src: the spatial variance estimate's
    sources (s, m1, m2), needed when min_samples > 0. -> (colour (h, w, 3) float32: what the pass stores, `written` (h, w) bool)."""
    c, V, A = np.asarray(c, F32), np.asarray(V, F32), np.asarray(A, F32)
    sig = {k: sigmas.get(k, D.DEFAULTS[k]) for k in SIGMAS}
    x, Vx = c, V
    if demod:
        x, Vx, _ = DM.demodulate(c, V, A, cov)
    if min_samples:
        Vx = SV.estimate(x, Vx, N, Z, A, cov, *src, min_samples, demod=demod, **sig)
    valid = (np.asarray(cov) > 0) & np.all(np.isfinite(x), axis=-1)  # the filter branch: the pass's own input
    Af = np.where(np.isfinite(A), A, F32(0)) if demod else A
    x1, _ = D.atrous_pass(x, Vx, N, Z, Af, cov, 1, sig["sigma_luminance"], sig["sigma_normal"], sig["sigma_depth"],
                          DM.NO_ALBEDO if demod else sig["sigma_albedo"])
    changed = np.any(np.asarray(x1, np.float64) != x.astype(np.float64), axis=-1)
    x1 = np.asarray(x1, F32)
    with np.errstate(all="ignore"):
        value = (x1 * DM.divisor(Af)[0]).astype(F32) if demod else x1
        N32 = np.asarray(N, F32)
        nn = (N32[..., 0] * N32[..., 0] + N32[..., 1] * N32[..., 1]) + N32[..., 2] * N32[..., 2]
        lp = D.lum(np.where(valid[..., None], x, F32(0)))
    centre = (nn > 0) & np.isfinite(np.asarray(Z, F32)) & np.isfinite(lp) & (demod | np.all(np.isfinite(A), axis=-1))
    written = valid & (changed | centre) & np.all(np.isfinite(value), axis=-1)
    return np.where(written[..., None], value, c).astype(F32), written


def feed_back(setup, iterations=5, demod=False, min_samples=0, **sigmas):
    """setup: a temporal set-up's dict (c, V, commit, cur; temporal_ref.integrate's layout). -> the staging set a clear commits
    with the switch on: setup['commit'] with the colour pass 1 stores, and 'written' (h, w) bool. iterations 0: the set-up's own."""
    commit = dict(setup["commit"])
    shape = np.asarray(setup["V"]).shape
    if iterations < 1:
        commit["written"] = np.zeros(shape, bool)
        return commit
    cur = setup["cur"]
    src = SV.sources_staged(setup["commit"]) if min_samples else None
    colour, written = pass1_colour(setup["c"], setup["V"], cur["N"], cur["Z"], cur["A"], cur["cov"], src, demod=demod and iterations >= 1,
                                   min_samples=min_samples, **sigmas)
    assert np.array_equal(np.asarray(setup["c"], F32).view(np.uint32), np.asarray(setup["commit"]["colour"], F32).view(np.uint32))  # the staged colour is the set-up's
    commit["colour"], commit["written"] = colour, written
    return commit


def temporal_setup(canvas, inputs, F, hist, cam_rd, iterations=5, demod=False, min_samples=0, gamma=0.0, rescale=False, sigmas=None, **kw):
    """history_clamp_ref.temporal_setup (its arguments in kw: the thresholds, ids, table, ...; gamma 0: no clamp; rescale: history
    illumination) followed by the feedback. -> its dict with 'commit_fb' = feed_back()'s set."""
    out = HC.temporal_setup(canvas, inputs, F, hist, cam_rd, gamma, rescale=rescale, sigmas=sigmas, **kw)
    out["commit_fb"] = feed_back(out, iterations, demod=demod, min_samples=min_samples, **(sigmas or {}))
    return out
