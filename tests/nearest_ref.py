"""numpy float32 restatement of the nearest-surface queries (include/srt_abi.h "nearest-surface queries"): the three distance
functions and the brute-force minimum over a scene's primitives. Written from the ABI text; never calls the library. Every
product, sum, quotient and square root is one float32 numpy operation, in the header's order, so the results are the bits the
contract asks for. A plain module, not a test module (tests/test_nearest_reference.py, tests/test_gpu_nearest.py).

Scene inputs come from records.py. A model's world record {v0, e1, e2} is the pre-pass's: v = ((m0 * x + m1 * y) + m2 * z) + m3 * 1,
the kernels' left-associated order (records.transform_points is the HOST's order, (m0 x + m1 y) + (m2 z + m3), which rounds
differently under a rotation: the blob968 case would miss by an ulp with it), e1 and e2 float32 differences."""
import numpy as np

from simple_raytracer_amd import records as R

F = np.float32
BACK, FEATURE_SHIFT = R.NEAREST_BACK, R.NEAREST_FEATURE_SHIFT


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _f(x):
    return np.asarray(x, F)


def sphere(c, radius, q):
    """-> distance, point (..., 3), flags; arguments broadcast against each other"""
    c, q = _f(c), _f(q)
    with np.errstate(all="ignore"):
        r = np.abs(_f(radius))
        v = q - c
        ln = np.sqrt(dot3(v, v))
        dist = np.abs(ln - r)
        s = r / ln
        zero = np.zeros_like(r)
        at_centre = c + np.stack(np.broadcast_arrays(r, zero, zero), -1)
        point = np.where((ln > 0)[..., None], c + v * s[..., None], at_centre)
    return dist.astype(F), point.astype(F), np.where(ln < r, BACK, 0).astype(np.uint32)


def plane(p, n, q):
    p, n, q = _f(p), _f(n), _f(q)
    with np.errstate(all="ignore"):
        nn = dot3(n, n)
        k = dot3(q - p, n)
        dist = np.abs(k / np.sqrt(nn))
        s = k / nn
        point = q - n * s[..., None]
    return dist.astype(F), point.astype(F), np.where(k < 0, BACK, 0).astype(np.uint32)


def triangle(wtri, q):
    """wtri (..., 9) = {v0, e1, e2}; Ericson 5.1.5, the regions in the header's order"""
    wtri, q = _f(wtri), _f(q)
    a, ab, ac = wtri[..., 0:3], wtri[..., 3:6], wtri[..., 6:9]
    with np.errstate(all="ignore"):
        ap = q - a
        d1, d2 = dot3(ab, ap), dot3(ac, ap)
        bp = ap - ab
        d3, d4 = dot3(ab, bp), dot3(ac, bp)
        cp = ap - ac
        d5, d6 = dot3(ab, cp), dot3(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [
            (d1 <= 0) & (d2 <= 0),
            (d3 >= 0) & (d4 <= d3),
            (vc <= 0) & (d1 >= 0) & (d3 <= 0),
            (d6 >= 0) & (d5 <= d6),
            (vb <= 0) & (d2 >= 0) & (d6 <= 0),
            (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0),
        ]
        codes = [1, 2, 4, 3, 5, 6]
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = F(1) / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        shape = np.broadcast(a, q).shape
        bc = lambda x: np.broadcast_to(x, shape)
        points = [
            bc(a),
            bc(a + ab),
            bc(a + ab * v_ab[..., None]),
            bc(a + ac),
            bc(a + ac * w_ac[..., None]),
            bc((a + ab) + (ac - ab) * w_bc[..., None]),
        ]
        face = bc((a + ab * v[..., None]) + ac * w[..., None])
        point = np.stack([np.select(conds, [pt[..., k] for pt in points], face[..., k]) for k in range(3)], -1).astype(F)
        feature = np.select(conds, codes, 0).astype(np.uint32)
        d = q - point
        dist = np.sqrt(dot3(d, d))
        nrm = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                        ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
        back = dot3(d, nrm) < 0
    return dist.astype(F), point, (np.where(back, BACK, 0).astype(np.uint32) | (feature << np.uint32(FEATURE_SHIFT))).astype(np.uint32)


def world_records(shape, tris):
    """the pre-pass's {v0, e1, e2} of a model's triangles -> (n, 9) float32"""
    first, n = int(shape["triangle_index"]), int(shape["num_triangles"])
    m = np.asarray(shape["transform"], F)
    pos = np.asarray(tris["v"]["pos"][first:first + n], F).reshape(n, 3, 3)
    x, y, z = pos[..., 0:1], pos[..., 1:2], pos[..., 2:3]
    with np.errstate(all="ignore"):
        w = ((m[0][None, None, :3] * x + m[1][None, None, :3] * y) + m[2][None, None, :3] * z) + m[3][None, None, :3] * F(1)
        w = w.astype(F)
        return np.concatenate([w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]], -1).astype(F)


def brute_force(shapes, tris, queries, skip_shape=None, tri_materials=None):
    """records.NEAREST per records.POINT_QUERY: the minimum over every primitive in (shape, triangle) order, the first of equal
    distances, strictly below max_distance; NaN distances never; hostile queries as the header says."""
    shapes = R.as_records(shapes, R.SHAPE)
    queries = R.as_records(queries, R.POINT_QUERY)
    q = queries["point"].astype(F)[:, None, :]  # (Q, 1, 3)
    dist, point, flags, shape_of, tri_of = [], [], [], [], []
    for i, s in enumerate(shapes):
        if skip_shape is not None and i == skip_shape:
            continue
        t = int(s["type"])
        if t == R.SHAPE_SPHERE:
            d, p, f = sphere(s["sphere_position"][None, None, :], np.asarray(s["sphere_radius"], F)[None, None], q)
            n_p = 1
        elif t == R.SHAPE_PLANE:
            d, p, f = plane(s["plane_position"][None, None, :], s["plane_normal"][None, None, :], q)
            n_p = 1
        elif t == R.SHAPE_MODEL:
            n_p = int(s["num_triangles"])
            if n_p == 0:
                continue
            d, p, f = triangle(world_records(s, tris)[None, :, :], q)
        else:
            continue
        dist.append(np.broadcast_to(d, (len(queries), n_p)))
        point.append(np.broadcast_to(p, (len(queries), n_p, 3)))
        flags.append(np.broadcast_to(f, (len(queries), n_p)))
        shape_of += [i] * n_p
        tri_of += list(range(n_p)) if t == R.SHAPE_MODEL else [R.HIT_NONE] * n_p
    out = np.zeros(len(queries), R.NEAREST)
    out["distance"], out["shape"], out["triangle"], out["material"] = np.inf, R.HIT_NONE, R.HIT_NONE, -1
    maxd = queries["max_distance"]
    invalid = ~np.isfinite(queries["point"]).all(-1) | np.isnan(maxd)
    out["flags"][invalid] = R.NEAREST_INVALID
    if not dist or not len(queries):
        return out
    dist, point, flags = np.concatenate(dist, 1), np.concatenate(point, 1), np.concatenate(flags, 1)
    shape_of, tri_of = np.asarray(shape_of, np.uint32), np.asarray(tri_of, np.uint32)
    best = np.argmin(np.where(np.isnan(dist), np.inf, dist), axis=1)  # the first of equal minima: the lower (shape, triangle)
    rows = np.arange(len(queries))
    bd = dist[rows, best]
    with np.errstate(invalid="ignore"):
        found = ~invalid & (maxd > 0) & (bd < maxd)
    for k in np.nonzero(found)[0]:
        b = best[k]
        si, ti = int(shape_of[b]), int(tri_of[b])
        mat = int(shapes[si]["material"])
        if tri_materials is not None and ti != R.HIT_NONE and mat >= 0:
            tm = int(tri_materials[int(shapes[si]["triangle_index"]) + ti])
            mat = tm if tm >= 0 else mat
        out[k] = (bd[k], si, ti, mat, point[k, b], R.NEAREST_FOUND | int(flags[k, b]))
    return out


def words(records):
    """(n, 8) uint32: every word of every record, what the tests compare"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)
