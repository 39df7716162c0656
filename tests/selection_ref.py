"""The selection overlay restated in numpy from its definition (include/srt_abi.h "selection overlay and the ID pass"): mask,
squared distance, alpha table, alpha plane and composite. Integer arithmetic but for the table, which is double. A plain module,
not a test module; written from the definition, not from the kernel (no tiles, no words, no early exits)."""
import math

import numpy as np

NONE = 1 << 30  # "no selected pixel within the radius"


def radius(width):
    """R = ceil(width + 0.5) - 1 for the float32 width"""
    return int(math.ceil(float(np.float32(width)) + 0.5)) - 1


def table(width, outline_alpha):
    """table[d2] = floor(clamp(width + 0.5 - sqrt(d2), 0, 1) * outline_alpha + 0.5), d2 = 0 .. 2 R^2 -> (uint8 array, R)"""
    w, R = float(np.float32(width)), radius(width)
    out = [int(math.floor(min(max(w + 0.5 - math.sqrt(float(d2)), 0.0), 1.0) * float(outline_alpha) + 0.5)) for d2 in range(2 * R * R + 1)]
    return np.array(out, np.uint8), R


def mask(shape_plane, selected, n_shapes):
    """m(p) = 1 where the ID plane's shape is in the set; indices beyond the scene never match"""
    sel = [int(s) for s in selected if 0 <= int(s) < n_shapes]
    return np.isin(shape_plane, np.array(sel, np.uint32)) if sel else np.zeros(shape_plane.shape, bool)


def distance2(m, R):
    """d2(p): the smallest dx^2 + dy^2 over q = p + (dx, dy), |dx|, |dy| <= R, q inside the frame, m(q) = 1; NONE without one"""
    h, w = m.shape
    d2 = np.full((h, w), NONE, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue  # every q is outside the frame
            # q = p + (dx, dy): the mask shifted so that entry p holds m(q), False outside the frame
            shifted = np.zeros((h, w), bool)
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yq, xq = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            shifted[ys, xs] = m[yq, xq]
            d2 = np.where(shifted, np.minimum(d2, dx * dx + dy * dy), d2)
    return d2


def alpha_plane(m, width, outline_alpha, fill_alpha):
    """alpha(p) (uint8) and the bool plane of the pixels that take the outline's colour (the others with alpha take the fill's)"""
    tab, R = table(width, outline_alpha)
    d2 = distance2(m, R)
    outline = ~m & (d2 != NONE)
    a = np.zeros(m.shape, np.uint8)
    a[m] = fill_alpha
    a[outline] = tab[d2[outline]]
    return a, outline


def composite(argb, a, outline, outline_argb, fill_argb):
    """out = (byte * (255 - a) + colour * a + 127) // 255 per colour byte of the (h, w, 4) A, R, G, B picture; the alpha byte stays,
    pixels with a == 0 keep their bytes"""
    out = argb.astype(np.int64).copy()
    al = a.astype(np.int64)
    for c in (1, 2, 3):
        colour = np.where(outline, int(outline_argb[c]), int(fill_argb[c])).astype(np.int64)
        mixed = (out[..., c] * (255 - al) + colour * al + 127) // 255
        out[..., c] = np.where(al != 0, mixed, out[..., c])
    return out.astype(np.uint8)


def apply(argb, shape_plane, selected, n_shapes, width, outline_argb, fill_argb):
    """the overlaid picture and the alpha plane for the resolved bytes `argb` (h, w, 4) and the ID pass's shape plane (h, w)"""
    m = mask(shape_plane, selected, n_shapes)
    a, outline = alpha_plane(m, width, int(outline_argb[0]), int(fill_argb[0]))
    return composite(argb, a, outline, outline_argb, fill_argb), a, m
