"""Exposure for the resolve (include/srt_abi.h srt_set_exposure; simple-raytracer_amd/csrc/exposure.hip) restated in numpy: the
bin rule, the trimmed mean in float64 in ascending bin order, the adaptation step and the exposed bytes. A plain module, not a
test module. The byte step is tests/denoise_ref.py's tonemap, the restatement the tonemap-edge tests hold the resolve to.

Everything here follows the header's text, never a device result. The integer parts (bins, counts, the kept window) are exact;
the scalar is float64 rounded to float32 where the header says so.
"""
import numpy as np

import denoise_ref as D

F32 = np.float32
BINS = 256
DEFAULTS = dict(mode=1, ev=0.0, key=0.18, low_permille=100, high_permille=950, adapt=1.0, min_ev=-16.0, max_ev=16.0)


def divided(source, ticks):
    """(n, 3) float32: source[..., :3] / (float)ticks; ticks None: an image that is divided already (the denoiser's)."""
    c = np.asarray(source, F32).reshape(-1, np.shape(source)[-1])[:, :3]
    if ticks is None:
        return c
    with np.errstate(all="ignore"):
        return (c / F32(np.uint32(ticks))).astype(F32)


def luminance(source, ticks):
    with np.errstate(all="ignore"):
        return D.lum(divided(source, ticks))


def bins_of(L):
    """Bin of every finite L > 0 (int64), four per octave over 2^-32 .. 2^32 from the bit pattern; -1: the pixel is left out."""
    L = np.asarray(L, F32)
    with np.errstate(all="ignore"):
        metered = np.isfinite(L) & (L > 0)
    b = (L.view(np.uint32).astype(np.int64) >> 21) - ((127 - 32) << 2)
    return np.where(metered, np.clip(b, 0, BINS - 1), -1)


def histogram(source, ticks):
    """-> hist (256 uint32), (metered, left out)"""
    b = bins_of(luminance(source, ticks))
    hist = np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)
    return hist, (int(hist.sum()), int(np.sum(b < 0)))


def window(N, low_permille, high_permille):
    """The kept pixels [lo, hi) of N metered ones in ascending luminance: at least one."""
    lo = N * int(low_permille) // 1000
    return lo, max(N * int(high_permille) // 1000, lo + 1)


def trimmed_mean(hist, low_permille, high_permille):
    """Mean log2 luminance (float64) of the kept pixels by their bin's centre, accumulated in ascending bin order; None: N == 0."""
    N = int(np.sum(hist.astype(np.int64)))
    if N == 0:
        return None
    lo, hi = window(N, low_permille, high_permille)
    total, mass, first = np.float64(0), 0, 0
    for k in range(BINS):
        last = first + int(hist[k])
        kept = min(last, hi) - max(first, lo)
        if kept > 0:
            total = total + np.float64(kept) * ((np.float64(k) + 0.5) / 4.0 - 32.0)
            mass += kept
        first = last
    return total / np.float64(mass)


class Meter:
    """The adaptation state of one handle across frames (float32, 0 and 'none yet' on a fresh handle) and the meter's step."""

    def __init__(self, **params):
        self.p = dict(DEFAULTS, **params)
        self.state, self.have_state = F32(0), False

    def reset(self):
        self.state, self.have_state = F32(0), False

    def frame(self, hist):
        """One metered frame -> (log2_exposure, exposure), float32."""
        p = self.p
        mean = trimmed_mean(np.asarray(hist), p["low_permille"], p["high_permille"])
        if mean is not None:
            target = np.log2(np.float64(F32(p["key"]))) - mean
            target = min(max(target, np.float64(F32(p["min_ev"]))), np.float64(F32(p["max_ev"])))
            s = np.float64(self.state)
            self.state = F32(s + (target - s) * np.float64(F32(p["adapt"])) if self.have_state else target)
            self.have_state = True
        l2 = F32(np.float64(self.state) + np.float64(F32(p["ev"])))
        return l2, F32(np.exp2(np.float64(l2)))


def manual(ev):
    """MANUAL mode -> (log2_exposure, exposure), float32."""
    ev = F32(ev)
    return ev, F32(np.exp2(np.float64(ev)))


def exposed_bytes(source, ticks, exposure):
    """(n, 4) uint8 A, R, G, B: tonemap(c * e) per channel of the divided colour, float32 products."""
    with np.errstate(all="ignore"):
        return D.tonemap((divided(source, ticks) * F32(exposure)).astype(F32))


def ulps(a, b):
    """Distance of two finite float32 in units of the last place (ordered bit patterns)."""
    def key(x):
        i = int(np.asarray(x, F32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))
