"""Bloom for the resolve (include/srt_abi.h srt_set_bloom; simple-raytracer_amd/csrc/bloom.hip) restated in numpy float32: the
prefilter, the reduce and expand filters with the header's parenthesisation, the pyramid and the composited bytes. A plain
module, not a test module. The byte step is tests/denoise_ref.py's tonemap, the luminance its lum.

Everything here follows the header's text, never a device result. Every constant is np.float32, so nothing is promoted to
float64; images are (h, w, 3) float32, horizontal is axis 1.
"""
import numpy as np

import denoise_ref as D

F32 = np.float32
MAX_LEVELS = 8
DEFAULTS = dict(threshold=1.0, knee=0.5, intensity=0.1, scatter=0.7, clamp=64.0, levels=6)


def params(**kw):
    """DEFAULTS overridden by kw, the floats as np.float32."""
    p = dict(DEFAULTS, **kw)
    return {k: (int(v) if k == "levels" else F32(v)) for k, v in p.items()}


def exposed(source, ticks, exposure=1.0):
    """x = (c / (float)ticks) * e per channel: (..., 3) float32; ticks None: an image that is divided already (divisor 1)."""
    c = np.asarray(source, F32)[..., :3]
    with np.errstate(all="ignore"):
        d = F32(1.0) if ticks is None else F32(np.uint32(ticks))
        return ((c / d).astype(F32) * F32(exposure)).astype(F32)


def soft_threshold(L, threshold, knee, clamp):
    """g of step 1 for finite luminances L > 0 (before the g > 0 test)."""
    L, T, K, Cl = np.asarray(L, F32), F32(threshold), F32(knee), F32(clamp)
    with np.errstate(all="ignore"):
        g = L - T
        if K > 0:
            s = np.clip((L - T) + K, F32(0), F32(2) * K)
            q = (s * s) / (F32(4) * K)
            g = np.maximum(g, q)
        if Cl > 0:
            g = np.minimum(g, Cl)
    return g.astype(F32)


def prefilter(x, threshold, knee, clamp):
    """Step 1: bright = x * (g / L) where the pixel is finite, L > 0 and g > 0; (0, 0, 0) elsewhere."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        L = D.lum(x)
        ok = np.isfinite(x).all(axis=-1) & np.isfinite(L) & (L > 0)
        g = soft_threshold(L, threshold, knee, clamp)
        ok = ok & (g > 0)
        k = (g / L).astype(F32)
        bright = (x * k[..., None]).astype(F32)
    return np.where(ok[..., None], bright, F32(0)).astype(F32)


def level_sizes(w, h, levels):
    """[(w_k, h_k)] of the effective levels: w_k = (w_{k-1} + 1) / 2, cut off after the first level that is 1 x 1."""
    out = []
    while len(out) < levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if (w, h) == (1, 1):
            break
    return out


def _reduce_axis(a, axis):
    n = a.shape[axis]
    i = np.arange((n + 1) // 2)
    t = [np.take(a, np.clip(2 * i - 1 + j, 0, n - 1), axis=axis) for j in range(4)]
    with np.errstate(all="ignore"):
        return (((t[0] + t[3]) + F32(3.0) * (t[1] + t[2])) * F32(0.125)).astype(F32)


def reduce(img):
    """Step 2: horizontal first (a w_k x h_{k-1} intermediate), then vertical."""
    return _reduce_axis(_reduce_axis(np.asarray(img, F32), 1), 0)


def _expand_axis(s, axis, n_dst):
    n = s.shape[axis]
    d = np.arange(n_dst)
    i = d // 2
    far = np.clip(np.where(d & 1, i + 1, i - 1), 0, n - 1)
    with np.errstate(all="ignore"):
        return (F32(0.75) * np.take(s, i, axis=axis) + F32(0.25) * np.take(s, far, axis=axis)).astype(F32)


def expand(s, w, h):
    """expand of step 3 to a w x h image: horizontal first, then vertical."""
    return _expand_axis(_expand_axis(np.asarray(s, F32), 1, w), 0, h)


def down_pyramid(x, p):
    x = np.asarray(x, F32)
    h, w = x.shape[:2]
    cur, down = prefilter(x, p["threshold"], p["knee"], p["clamp"]), []
    for _ in level_sizes(w, h, p["levels"]):
        cur = reduce(cur)
        down.append(cur)
    return down


def pyramid(x, p):
    """[up_0, up_1, ..] of the exposed image x (h, w, 3) under params() p: up_last = down_last, up_k = down_k + scatter *
    expand(up_{k+1})."""
    up = down_pyramid(x, p)
    with np.errstate(all="ignore"):
        for k in range(len(up) - 2, -1, -1):
            hk, wk = up[k].shape[:2]
            up[k] = (up[k] + p["scatter"] * expand(up[k + 1], wk, hk)).astype(F32)
    return up


def composite(x, up0, intensity):
    """Step 4: out = x + intensity * expand(up_0), (h, w, 3) float32."""
    x = np.asarray(x, F32)
    h, w = x.shape[:2]
    with np.errstate(all="ignore"):
        return (x + F32(intensity) * expand(up0, w, h)).astype(F32)


def bloomed_bytes(source, ticks, exposure, p):
    """(h, w, 4) uint8 A, R, G, B of the (h, w, >= 3) source; -> bytes, [up_k]."""
    x = exposed(source, ticks, exposure)
    up = pyramid(x, p)
    return D.tonemap(composite(x, up[0], p["intensity"])), up


def same_bits(got, want):
    """got == want as uint32 views, any NaN equal to any NaN."""
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool(np.where(nan, np.isnan(g), g.view(np.uint32) == w.view(np.uint32)).all())
