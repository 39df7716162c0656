"""numpy restatement of the sky lookup of an escaped path (csrc/device_shading.h sky_box, oracle/srt_oracle.c sky_box): the
image filter of OpenCL 3.0 section 8.2 for normalised coordinates, addressing CLAMP_TO_EDGE, filter LINEAR, under the
reference kernel's mapping of a direction to the image, in float32, unfused, every product and sum rounded on its own. Written
from the specification's words and from the reference kernel's mapping, not from either sampler's text; the CLAMP sibling of
tests/texture_ref.py (addressing REPEAT), whose host build of csrc/detmath.h it shares: atan2pif, bilinear and, here, dot3 and
powi come through texture_ref.lib(). A plain module, not a test module.

The rule, for an image of W x H texels (row 0 = bottom, v = 0) and a direction d:

    u = atan2pi(d.z, d.x) * 0.5 + 0.5           v = d.y * 0.5 + 0.5
    fu = u * W - 0.5                            fv = v * H - 0.5
    i0 = floor(fu), a = fu - i0                 j0 = floor(fv), b = fv - j0
    i1 = i0 + 1, both clamped to [0, W - 1]     j1 = j0 + 1, both clamped to [0, H - 1]
    colour.c = dm_bilinear((1-a)(1-b), T[j0,i0].c,  a(1-b), T[j0,i1].c,  (1-a)b, T[j1,i0].c,  ab, T[j1,i1].c)   c = r, g, b
    sky_box = colour + sun

The alpha lane of a texel takes no part. The seam of the mapping is the half plane x < 0, z = 0: u = 1 on its +0 side and u = 0
on its -0 side, and the filter clamps there, it does not wrap.

THE SUN LOBE is restated for an integer sun_focus of 1 .. 32 only (dm_powf's dm_powi path, which the library's default of 25
takes): sun = (sun_color * powi(max(dot(d, -sun_direction), 0), focus)) * sun_intensity, max as `x < 0 ? 0 : x`. Any other
focus raises. With sun_intensity = 0 the lobe still counts: it turns -0 into +0 and a NaN direction into NaN.

COORDINATES THAT ARE NOT FINITE, as the code has them (the specification leaves the conversion of such a floor to an integer
undefined; both samplers pin it the same way). A unit direction keeps u and v in [0, 1], so fu lies in [-0.5, W - 0.5] and none
of this applies; it takes a NaN or infinite direction component.
  * NaN (a NaN component of the direction: atan2pi gives NaN, so does d.y * 0.5): the floor is taken as 0, a = NaN - 0 = NaN;
    the texels read are (0, 1) clamped, every weight is NaN and so is every channel.
  * +inf / -inf (d.y infinite): the floor is taken as that of the coordinate clamped to [-1, W] (rows: [-1, H]): W or -1, so
    both indices clamp to the last or the first texel; a = fu - floor is +inf or -inf (it is NOT reduced to a fraction), the
    weights are infinities and NaNs (inf * 0 where the other axis's fraction is 0) and no channel is a number one would want.
  * The zero direction (normalize(0) = 0, components +0 or -0) is finite: atan2pi(+-0, +0) = +-0, atan2pi(+-0, -0) = +-1, so
    u is 0.5, 0 or 1 by the signs of the zeros, and v = 0.5: the middle row, at the seam or opposite it.

sample() and sky_box() take a `mutant`: one named slip of the rule (MUTANTS), for tests/test_sky_cases.py to show that the
skies and cameras of tests/sky_cases.py tell each of them from the rule."""
import ctypes as C

import numpy as np

import texture_ref as TR

F = np.float32
MUTANTS = ("repeat", "clamp_to_w", "a_from_clamped", "round", "truncate", "scale_w_minus_1", "w10_w01_swapped", "rows_flipped",
           "xy_swapped", "alpha_added")


def _lib():
    lib = TR.lib()
    lib.tex_dot3.restype = None
    lib.tex_powi.restype = None
    return lib


def dot3(a, b):
    """a (n, 3), b (3,) -> dm_dot3 per row"""
    a, b = np.ascontiguousarray(a, F).reshape(-1, 3), np.ascontiguousarray(b, F).reshape(3)
    out = np.zeros(len(a), F)
    _lib().tex_dot3(TR._p(a), TR._p(b), TR._p(out), C.c_size_t(len(a)))
    return out


def powi(x, e):
    x = np.ascontiguousarray(x, F).reshape(-1)
    out = np.zeros(len(x), F)
    _lib().tex_powi(TR._p(x), C.c_int(int(e)), TR._p(out), C.c_size_t(len(x)))
    return out


def uv(dirs):
    """dirs (n, 3) -> u, v (n,) float32"""
    d = np.asarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = TR.atan2pif(d[:, 2], d[:, 0]) * F(0.5) + F(0.5)
        v = d[:, 1] * F(0.5) + F(0.5)
    return u.astype(F), v.astype(F)


def _axis(coord, n, mutant, axis):
    """One axis of the filter: coordinate (n,) in [0, 1] -> unclamped floor (int64), the two texel indices, the fraction."""
    with np.errstate(all="ignore"):
        scale = F(n - 1) if mutant == "scale_w_minus_1" else F(n)
        f = (coord * scale - F(0.5)).astype(F)
        if mutant == "round":
            lo = np.rint(f)
        elif mutant == "truncate":
            lo = np.trunc(f)
        else:
            lo = np.floor(f)
        lo = np.where(np.isnan(f), F(0), np.clip(lo, F(-1), F(n))).astype(F)  # (only a coordinate that is not finite is moved)
        frac = (f - lo).astype(F)
        i0 = lo.astype(np.int64)
        i1 = i0 + 1
        if mutant == "repeat":
            c0, c1 = np.mod(i0, n), np.mod(i1, n)
        elif mutant == "clamp_to_w":
            c0, c1 = np.clip(i0, 0, n), np.clip(i1, 0, n)
        else:
            c0, c1 = np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1)
        if mutant == "a_from_clamped":
            frac = (np.clip(f, F(0), F(n - 1)) - c0.astype(F)).astype(F)
    return i0, c0, c1, frac


def footprint(image, dirs):
    """-> dict: x0, y0 (the floors before the clamp), i0, i1, j0, j1 (after it), u, v; what the coverage tests count"""
    H, W = np.asarray(image).shape[:2]
    u, v = uv(dirs)
    x0, i0, i1, _ = _axis(u, W, None, 0)
    y0, j0, j1, _ = _axis(v, H, None, 1)
    return {"x0": x0, "y0": y0, "i0": i0, "i1": i1, "j0": j0, "j1": j1, "u": u, "v": v}


def sample(image, u, v, mutant=None):
    """image (H, W, 4) float32, row 0 = bottom; u, v (n,) -> (n, 3) float32"""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    u, v = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    _, i0, i1, a = _axis(u, W, mutant, 0)
    _, j0, j1, b = _axis(v, H, mutant, 1)
    if mutant == "rows_flipped":
        j0, j1 = H - 1 - j0, H - 1 - j1
    # texel (i, j) lies at j * W + i; an index past the image (clamp_to_w alone) reads a texel of zeros behind it
    flat = np.concatenate([image.reshape(-1, 4), np.zeros((W + 1, 4), F)])
    if mutant == "xy_swapped":
        at = lambda i, j: flat[i * H + j]
    else:
        at = lambda i, j: flat[j * W + i]
    T = [at(i0, j0), at(i1, j0), at(i0, j1), at(i1, j1)]
    one = F(1)
    with np.errstate(all="ignore"):
        w = [(one - a) * (one - b), a * (one - b), (one - a) * b, a * b]
        if mutant == "w10_w01_swapped":
            w[1], w[2] = w[2], w[1]
        w = np.stack(w, axis=1).astype(F)
        out = np.zeros((len(u), 3), F)
        for c in range(3):
            out[:, c] = TR.bilinear(w, np.stack([t[:, c] for t in T], axis=1))
        if mutant == "alpha_added":
            out = (out + TR.bilinear(w, np.stack([t[:, 3] for t in T], axis=1))[:, None]).astype(F)
    return out


def sun(sd, dirs):
    """The sun lobe of records.SCENE_DATA sd for dirs (n, 3) -> (n, 3); integer sun_focus 1 .. 32 only."""
    focus = float(sd["sun_focus"])
    if not (1.0 <= focus <= 32.0 and focus == int(focus)):
        raise ValueError(f"the sun lobe is restated for an integer sun_focus of 1 .. 32, not {focus}")
    d = np.asarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = dot3(d, -np.asarray(sd["sun_direction"], F).reshape(-1)[:3])
        x = np.where(x < F(0), F(0), x).astype(F)
        lobe = powi(x, int(focus))
        colour = np.asarray(sd["sun_color"], F).reshape(-1)[:3]
        return ((colour[None, :] * lobe[:, None]).astype(F) * F(sd["sun_intensity"])).astype(F)


def sky_box(sd, image, dirs, mutant=None):
    """sky_box of every direction: (n, 3) float32"""
    u, v = uv(dirs)
    with np.errstate(all="ignore"):
        return (sample(image, u, v, mutant) + sun(sd, dirs)).astype(F)


def frame(sd, image, dirs, mutant=None):
    """What one sample of an empty scene adds to a cleared canvas: (0 + 1 * sky_box) / 1 added to 0 -- sky_box + 0."""
    with np.errstate(all="ignore"):
        return (sky_box(sd, image, dirs, mutant) + F(0)).astype(F)
