"""The crafted canvas of tests/test_tonemap_cases.py and tests/test_gpu_tonemap_edges.py: canvas values on and around every place
where the resolve's byte changes, and the non-finite edges. A plain module, not a test module.

The resolve is canvas / ticks -> ACES fit -> sqrt -> * 255 -> truncate (render.cl:473-481,525-535); byte() below is
tests/denoise_ref.py's float32 restatement of it for one channel. The set is made from that CPU reference alone, never from a
GPU result, and is deterministic: no random numbers.

  boundary windows  for every byte k = 1..255 the smallest float x in (0, 100] that bisection over the bit patterns finds with
                    byte(x) >= k, and every float within +-64 ulps of it (255 x 129 values)
  divided windows   float32(w * float32(ticks)) of the +-8 ulp windows w for ticks 3, 7, 10, 16777217 (-> 2^24) and 4294967295
                    (-> 2^32): after the device's division they land on and around the boundaries
  edges             signed zeros, denormals, FLT_MIN, small negatives, the overflow of x * x * 2.51 near 1.2e19, FLT_MAX, +-inf, NaNs

image() packs a list of values into R, G and B with the list rotated by one third per channel, so every value meets every
channel, and fills the alpha lane with garbage (NaN and 1e30) that must never reach a byte.
"""
import functools

import numpy as np

import denoise_ref as D

F32 = np.float32
TICKS = (1, 3, 7, 10, 0, 16777217, 4294967295)          # every divisor the tests resolve with
DIVIDED_TICKS = (3, 7, 10, 16777217, 4294967295)        # those with divided windows of their own
WIDE, NARROW = 64, 8                                    # half widths of the windows, in ulps
WIDTH = 211                                             # of natural_image(): odd, no multiple of a 16-pixel tile
BLOCK = 256                                             # threads of a resolve block
LARGE_PIXELS = 4096 * BLOCK + 257                       # past srt_resolve_kernel's grid cap: the grid-stride loop runs twice


def f32_ticks(ticks):
    """(float)num_steps of a uint32, round to nearest even: 16777217 -> 2^24, 4294967295 -> 2^32."""
    return F32(np.uint32(ticks))


def byte(x):
    """The resolve's byte of already divided channel values (float32 steps, tests/denoise_ref.py)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return D._to_uchar(np.sqrt(D._aces1(x)) * F32(255.0))


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def boundaries():
    """uint32 bit patterns b[k - 1], k = 1..255: byte(float(b)) >= k and byte(float(b - 1)) < k, found by bisection between the
    smallest denormal and 100.0. (The byte is not monotone within a few ulps of a boundary, so this is one crossing of possibly
    several; the windows around it hold the others.)"""
    ks = np.arange(1, 256)
    lo = np.full(255, 1, np.uint32)                       # byte(smallest denormal) = 0 < k
    hi = np.full(255, int(_bits(F32(100.0))), np.uint32)  # byte(100) = 255 >= k
    assert np.all(byte(lo.view(F32)) < ks) and np.all(byte(hi.view(F32)) >= ks)
    while np.any(hi - lo > 1):
        mid = lo + (hi - lo) // 2
        up = byte(mid.view(F32)) >= ks
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return hi


def windows(half):
    """Every float within +-half ulps of each boundary: (255, 2 half + 1) float32, all positive and finite."""
    b = boundaries().astype(np.int64)[:, None] + np.arange(-half, half + 1)[None, :]
    assert b.min() > 0 and b.max() < 0x7F800000
    return b.astype(np.uint32).view(F32)


def divided_windows(ticks):
    """float32(w * float32(ticks)) of the +-8 ulp windows."""
    with np.errstate(all="ignore"):
        return (windows(NARROW) * f32_ticks(ticks)).astype(F32)


def edges():
    """The non-finite and tiny ends, as bit patterns where the value matters to the bit."""
    fi = np.finfo(F32)
    pos = [0.0, float(fi.smallest_subnormal), float(np.uint32(0x007FFFFF).view(F32)), float(fi.tiny),  # 0, denormals, FLT_MIN
           1e19, 1.16e19, 1.18e19, 1.2e19, float(fi.max), np.inf]
    vals = np.asarray(pos + [-0.012, -0.0119, -1e-3], F32)
    signed = np.concatenate([vals, -vals[:len(pos)]])
    nans = np.asarray([0x7FC00000, 0xFFC00000, 0x7FC12345], np.uint32).view(F32)  # quiet NaNs of both signs, one with a payload
    return np.concatenate([signed, nans]).astype(F32)


def _pad(v, multiple):
    """v followed by 1.0s up to a multiple of `multiple` values."""
    n = -len(v) % multiple
    return np.concatenate([v, np.ones(n, F32)]) if n else v


@functools.lru_cache(maxsize=None)
def values():
    """The whole crafted list (float32, read-only): boundary windows, divided windows, edges; padded with 1.0 to WIDTH rows."""
    v = np.concatenate([windows(WIDE).ravel()] + [divided_windows(t).ravel() for t in DIVIDED_TICKS] + [edges()])
    v = _pad(v, WIDTH)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def narrow_values():
    """The +-8 ulp subset with the divided windows and the edges: what the reference build's bytes are stored for."""
    v = np.concatenate([windows(NARROW).ravel()] + [divided_windows(t).ravel() for t in DIVIDED_TICKS] + [edges()])
    v.setflags(write=False)
    return v


def image(v):
    """(len(v), 4) float32 canvas pixels: R = v, G = v rotated by a third, B = v rotated by two thirds, so every value of v
    appears in every channel; alpha = NaN and 1e30 in turn."""
    v = np.asarray(v, F32)
    n = len(v)
    out = np.empty((n, 4), F32)
    for ch in range(3):
        out[:, ch] = np.roll(v, -(ch * n // 3))
    out[0::2, 3] = np.nan
    out[1::2, 3] = F32(1e30)
    return out


@functools.lru_cache(maxsize=None)
def natural_image():
    """(height, WIDTH, 4): image(values()), read-only."""
    a = image(values()).reshape(-1, WIDTH, 4)
    a.setflags(write=False)
    return a


def pixels(count):
    """`count` pixels (count, 4) of the crafted canvas: all of it, a spread of it (fewer), or it tiled (more)."""
    flat = natural_image().reshape(-1, 4)
    n = len(flat)
    if count <= n:
        return flat[np.linspace(0, n - 1, count).astype(np.int64)].copy() if count > 1 else flat[WIDE:WIDE + 1].copy()  # (1: byte 1's boundary itself)
    return np.tile(flat, (-(-count // n), 1))[:count].copy()


def same_canvas(got, want):
    """got == want bit for bit, where a NaN equals any NaN and a -0 of `want` may have become +0 (-0 + 0 = +0)."""
    g, w = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(w)
    minus_zero = w.view(np.uint32) == 0x80000000
    ok = np.where(nan, np.isnan(g), np.where(minus_zero, g == 0, g.view(np.uint32) == w.view(np.uint32)))
    return bool(ok.all())


def near_boundary(x, ulps=WIDE):
    """How many of the float32 values x lie within `ulps` ulps of a boundary of byte()."""
    b = np.sort(boundaries().astype(np.int64))
    x = np.asarray(x, F32).ravel()
    x = x[np.isfinite(x) & (x > 0)]
    xb = x.view(np.uint32).astype(np.int64)
    i = np.clip(np.searchsorted(b, xb), 1, len(b) - 1)
    return int(np.sum(np.minimum(np.abs(xb - b[i - 1]), np.abs(xb - b[i])) <= ulps))


# ---- the scene whose every path returns exactly +0: the camera inside a black sphere that emits nothing ----

def zero_scene():
    """shapes, tris, mats: every camera ray hits the inside of the sphere, the path's colour mask becomes (0, 0, 0), nothing
    emits, and the bounces end inside: radiance +0 in every channel."""
    from simple_raytracer_amd import records as R
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material((0.0, 0.0, 0.0))
    shapes = np.zeros(1, R.SHAPE)
    shapes[0] = R.sphere(0, (0.0, 0.5, 5.0), 10.0)  # scenes.default_camera() sits at its centre
    return shapes, R.box_triangles(), mats
