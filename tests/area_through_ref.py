"""The authority of the X-ray area selection tests (include/srt_abi.h "area selection, through"): per pixel of a frame the candidate
list of the pixel centre's ray from tests/multi_hit_ref.py -- the CPU oracle's own intersectors, never the library's answer to a
hit query -- under the mask of tests/area_ref.py, counted as the definition says. The rays themselves are data handed in: the GPU
tests take them from pick_rays (the ID pass's ray set-up, bit for bit), the host test from host_rays below.
A plain module, not a test module."""
import numpy as np

import area_ref as AR
import multi_hit_ref as M
from simple_raytracer_amd import records as R

F = np.float32


def pixel_centres(w, h):
    """(w * h, 2) float32: (px + 0.5, py + 0.5), row by row"""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(F)


def ray_valid(ray):
    """the cast's validity rule for a ray given with a unit direction: finite origin and direction, a direction that is not zero,
    a tmax that is a number"""
    o, d = np.asarray(ray["origin"], F), np.asarray(ray["direction"], F)
    return bool(np.isfinite(o).all() and np.isfinite(d).all() and d.any() and not np.isnan(ray["tmax"]))


def host_rays(rd):
    """the pixel centres' rays of a frame restated in float32 numpy, for choosing cameras WITHOUT a device. The device's set-up
    replaces the divisions by multiplications with correctly rounded reciprocals, so these agree with pick_rays to rounding, not
    bit for bit: they serve statements with slack (a pixel has three candidates), never an equality with the device."""
    w, h = int(rd["width"]), int(rd["height"])
    xy = pixel_centres(w, h)
    cam = np.asarray(rd["camera_to_world"], F)
    sx = ((F(2) * (xy[:, 0] / F(w)) - F(1)) * F(rd["aspect_ratio"])) * F(rd["fov_scale"])
    sy = (F(1) - F(2) * (xy[:, 1] / F(h))) * F(rd["fov_scale"])
    v = sx[:, None] * cam[0, :3] + sy[:, None] * cam[1, :3] - cam[2, :3]
    with np.errstate(all="ignore"):
        d = (v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(F)
    rays = np.zeros(w * h, R.RAY)
    rays["origin"], rays["direction"], rays["tmax"] = cam[3, :3], d, np.inf
    return rays


def candidate_lists(oracle, scn, rays):
    """per ray its ordered candidate list [(t, shape, triangle or None), ...]; a refused ray has none"""
    ref = M.Reference(oracle, *scn)
    return [ref.candidates(r["origin"], r["direction"], r["tmax"]) if ray_valid(r) else [] for r in rays]


def _summary(m, miss, counts, target):
    area = int(m.sum())
    return dict(area_pixels=area, hit_pixels=area - miss, miss_pixels=miss, distinct=int((counts > 0).sum()), target_pixels=(area - miss) if target else 0)


def coverage(lists, w, h, rect, lasso, n_shapes):
    """shape coverage, through -> (counts (n_shapes,) uint32, summary dict): a pixel counts a shape once"""
    m = AR.mask(rect, lasso, w, h).ravel()
    counts, miss = np.zeros(n_shapes, np.uint32), 0
    for q in np.flatnonzero(m):
        shapes = {c[1] for c in lists[q]}
        miss += not shapes
        for s in shapes:
            if s < n_shapes:
                counts[s] += 1
    return counts, _summary(m, miss, counts, False)


def triangle_coverage(lists, w, h, s0, n_tri, rect, lasso):
    """triangle coverage of model shape s0, through -> (counts (n_tri,) uint32, summary dict); target_pixels counts pixels"""
    m = AR.mask(rect, lasso, w, h).ravel()
    counts, miss = np.zeros(n_tri, np.uint32), 0
    for q in np.flatnonzero(m):
        tris = [c[2] for c in lists[q] if c[1] == s0]
        miss += not tris
        for k in tris:
            if k < n_tri:
                counts[k] += 1
    return counts, _summary(m, miss, counts, True)


def visible(lists, w, h, n_shapes):
    """the shape plane the oracle's lists imply: the first candidate's shape per pixel, AR.NONE where there is none -> (h, w)"""
    return np.array([cl[0][1] if cl else AR.NONE for cl in lists], np.uint32).reshape(h, w)


def sees_through(lists, w, h, n_shapes):
    """what every scene of the tests has to show: some pixel with at least 3 candidates, and a shape counted on more pixels
    through than visibly -> (most candidates on a pixel, the shapes with counts_through > counts_visible)"""
    through, _ = coverage(lists, w, h, (0, 0, w, h), None, n_shapes)
    vis, _ = AR.coverage(visible(lists, w, h, n_shapes), (0, 0, w, h), None, n_shapes)
    return max(len(cl) for cl in lists), np.flatnonzero(through > vis).tolist()
