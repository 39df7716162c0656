"""Area selection (include/srt_abi.h "area selection") restated in numpy from the definition, in int64: the mask of a rectangle and
a lasso over a frame, the coverage counts over ID planes (numpy.bincount), the selection modes, and the directed cases the host and
device tests share. A plain module, not a test module; it reads nothing of csrc/area_host.h."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_VERTICES, COORD_MAX = 256, 1 << 20
REPLACE, ADD, SUBTRACT, TOGGLE = 0, 1, 2, 3
W, H = 70, 37


def lasso_inside(vertices, w, h):
    """(h, w) bool: the even-odd rule on doubled coordinates, every pixel against every edge at once"""
    v = 2 * np.asarray(vertices, np.int64).reshape(-1, 2)
    cx = (2 * np.arange(w, dtype=np.int64) + 1)[None, :]
    cy = (2 * np.arange(h, dtype=np.int64) + 1)[:, None]
    odd = np.zeros((h, w), bool)
    for i in range(len(v)):
        (ax, ay), (bx, by) = v[i], v[(i + 1) % len(v)]
        spans = (ay < cy) != (by < cy)
        cross = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        counts = (cross > 0) if by > ay else (cross < 0)
        odd ^= spans & counts
    return odd


def mask(rect, lasso, w, h):
    """M(p): rectangle and frame and (no lasso or inside) -> (h, w) bool"""
    x0, y0, x1, y1 = rect
    ys, xs = np.mgrid[0:h, 0:w]
    m = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    if lasso is not None and len(lasso):
        m &= lasso_inside(lasso, w, h)
    return m


def summary(m, shape, counts, target=0):
    miss = int((m & (shape == NONE)).sum())
    return dict(area_pixels=int(m.sum()), hit_pixels=int(m.sum()) - miss, miss_pixels=miss, distinct=int((counts > 0).sum()), target_pixels=target)


def coverage(shape, rect, lasso, n_shapes):
    """(counts (n_shapes,) uint32, summary dict) of a shape plane"""
    h, w = shape.shape
    m = mask(rect, lasso, w, h)
    keys = shape[m & (shape != NONE)].astype(np.int64)
    counts = np.bincount(keys[keys < n_shapes], minlength=n_shapes).astype(np.uint32)
    return counts, summary(m, shape, counts)


def triangle_coverage(shape, triangle, s0, n_tri, rect, lasso):
    h, w = shape.shape
    m = mask(rect, lasso, w, h)
    keys = triangle[m & (shape == s0)].astype(np.int64)
    counts = np.bincount(keys[keys < n_tri], minlength=n_tri).astype(np.uint32)
    return counts, summary(m, shape, counts, int(counts.sum()))


def combine(current, counts, mode, min_pixels):
    """the new selection list, ascending and unique"""
    hit = set(np.nonzero(counts >= max(int(min_pixels), 1))[0].tolist())
    cur = set(int(s) for s in current)
    new = {REPLACE: hit, ADD: cur | hit, SUBTRACT: cur - hit, TOGGLE: cur ^ hit}[mode]
    return np.array(sorted(new), np.uint32)


def segments(rect, w, h):
    """the 64-pixel row segments the counting kernel's waves take inside rect clipped to the frame: (y, xa, xb) each"""
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], w), min(rect[3], h)
    return [(y, xa, min(xa + 64, x1)) for y in range(y0, y1) for xa in range(x0, x1, 64)]


def zigzag(n=MAX_VERTICES, x0=-300, x1=460, top=3, mid=20, bottom=34):
    """n vertices: a saw along the top (teeth between `top` and `mid`, about three pixels each, reaching past the frame on both sides),
    closed along the bottom"""
    k = n - 2
    xs = np.round(np.linspace(x0, x1, k)).astype(int)
    saw = [(int(x), top if i % 2 == 0 else mid) for i, x in enumerate(xs)]
    return saw + [(x1, bottom), (x0, bottom)]


FAR = COORD_MAX
# name -> lasso vertices (pixel-corner coordinates) on the 70 x 37 frame
LASSOS = {
    "convex": [(5, 3), (60, 8), (50, 33), (10, 30)],
    "concave_L": [(4, 2), (30, 2), (30, 18), (64, 18), (64, 35), (4, 35)],
    "concave_U": [(6, 3), (20, 3), (20, 25), (48, 25), (48, 3), (62, 3), (62, 34), (6, 34)],
    "bow_tie": [(5, 4), (65, 32), (65, 4), (5, 32)],
    "zero_area": [(10, 10), (40, 20), (10, 10), (40, 20)],
    "diagonal_through_centres": [(3, 3), (33, 33), (3, 33)],  # in doubled coordinates the edge x = y passes through every centre (2k + 1, 2k + 1)
    "half_pixel_diagonal": [(2, 1), (40, 20), (2, 30)],  # slope 1/2: centres on the edge every other pixel
    "far_outside": [(-FAR, -FAR), (FAR, -FAR + 3), (35, 18), (FAR, FAR), (-FAR, FAR - 7)],
    "far_sliver": [(-FAR, 5), (FAR, 6), (FAR, 30), (-FAR, 31)],
    "zigzag_256": zigzag(),
    "collinear_3": [(5, 5), (30, 30), (60, 60)],
    "triangle_ccw": [(8, 4), (12, 33), (66, 20)],
}
LASSOS["convex_reversed"] = LASSOS["convex"][::-1]
LASSOS["bow_tie_reversed"] = LASSOS["bow_tie"][::-1]
EMPTY = ("zero_area", "collinear_3")  # their masks are empty by the definition
# rectangles on the 70 x 37 frame: wholly inside, partly over each border, wholly outside, empty, the frame, beyond it on all sides
RECTS = {
    "frame": (0, 0, W, H), "inside": (7, 5, 51, 29), "one_pixel": (33, 17, 34, 18), "width_65": (3, 2, 68, 30), "odd_x": (11, 1, 63, 36),
    "over_left": (-9, 6, 20, 22), "over_top": (10, -4, 44, 9), "over_right": (50, 8, 90, 30), "over_bottom": (20, 25, 60, 70),
    "beyond": (-5, -5, W + 5, H + 5), "outside": (W + 1, 3, W + 30, 20), "outside_above": (3, -20, 40, 0), "empty_x": (20, 5, 20, 30),
    "empty_y": (5, 9, 40, 9), "empty_outside": (-7, -7, -7, -7),
}
