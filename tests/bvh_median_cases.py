"""What the median-order tests share (tests/test_bvh_median_host.py, tests/test_gpu_bvh_build_median.py): the case meshes, a numpy
statement of the order of include/srt_abi.h (SRT_BUILD_ORDER_MEDIAN) -- float32, level by level, np.argsort(kind="stable") --
and the number of launches the device needs, stated from SRT_BUILD_LOCAL and the count alone. A plain module, not a test
module."""
import numpy as np

import bvh_build_cases as B
import bvh_deform_cases as D
from simple_raytracer_amd import scenes as S, tracer as T

F = np.float32
FLT_MAX = B.FLT_MAX
NONFINITE = 0x10000
LEAF_MAX = 3
LOCAL = T.BUILD_LOCAL  # csrc/device_types.h SRT_BUILD_LOCAL
assert LOCAL == 1024
# no split (1, 3), the first split (4), ragged halves (5, 7, 8); a wave and a round of the local launch; the local launch alone
# against one global level; two ranges, ragged; two global levels with ranges of unequal size
PREFIXES = [1, 3, 4, 5, 7, 8, 64, 65, 257, LOCAL - 1, LOCAL, LOCAL + 1, 2 * LOCAL, 2 * LOCAL + 1, 4 * LOCAL + 3]
SAME = ["same257", f"same{LOCAL + 1}"]
# (model, variant): the prefixes, n6k itself (three global levels, ragged everywhere), hostile variants, coinciding centroids
CASES = ([(f"p{n}", "base") for n in PREFIXES] + [(m, v) for v in B.VARIANTS for m in D.SIZES if (v, m) != ("base", "n1")]
         + [(m, "base") for m in SAME])


def global_levels(n):
    """depths whose largest range, ceil(n / 2^L), exceeds LOCAL"""
    levels = 0
    while n > LOCAL << levels:
        levels += 1
    return levels


def launches(n):
    """per global level L an extents launch, a key launch and ceil((17 + L) / 8) passes of three launches; then the local one"""
    return sum(2 + 3 * ((17 + level + 7) // 8) for level in range(global_levels(n))) + 1


def median_order(shape, tris):
    """the definition: from the identity, every range of the balanced topology with more than three records sorted stably by its
    key, top-down"""
    lo, hi, finite = B.boxes(shape, tris)
    n = len(lo)
    with np.errstate(all="ignore"):
        c = F(0.5) * lo + F(0.5) * hi
    order = np.arange(n, dtype=np.uint32)
    ranges = [(0, n)]
    while ranges:
        halves = []
        for b, e in ranges:
            cnt = e - b
            if cnt <= LEAF_MAX:
                continue
            idx = order[b:e]
            fin, cc = finite[idx], c[idx]
            clo = cc[fin].min(axis=0) if fin.any() else np.full(3, FLT_MAX, F)
            chi = cc[fin].max(axis=0) if fin.any() else np.full(3, -FLT_MAX, F)
            with np.errstate(all="ignore"):
                ext = chi - clo
                a = 0
                for k in (1, 2):
                    if ext[k] > ext[a]:
                        a = k
                key = np.zeros(cnt, np.uint32)
                if ext[a] > 0 and np.isfinite(ext[a]):
                    f = (cc[:, a] - clo[a]) * (F(65536.0) / ext[a])
                    assert f.dtype == F
                    f = np.where(fin, f, F(0.0))
                    key = np.where(f >= F(65535.0), 65535, np.where(f > F(0.0), np.trunc(f), 0)).astype(np.uint32)
            key = np.where(fin, key, NONFINITE).astype(np.uint32)
            order[b:e] = idx[np.argsort(key, kind="stable")]
            halves += [(b, b + cnt // 2), (b + cnt // 2, e)]
        ranges = halves
    return order


def cost_meshes():
    """(name, model shape, triangles): the meshes whose tree costs are compared -- n200, n6k, the two 968-triangle instances of
    the bench's mesh scene, and the case prefixes with a tree worth the name"""
    out = [(m, D.shape_over(B.mesh(m)), B.mesh(m)) for m in ("n200", "n6k")]
    shapes, tris, _ = S.mesh_scene(2)
    out += [(f"mesh968[{k}]", s, tris) for k, s in enumerate(s for s in shapes if int(s["type"]) == 2 and int(s["num_triangles"]) == 968)]
    out += [(f"p{n}", D.shape_over(B.mesh(f"p{n}")), B.mesh(f"p{n}")) for n in PREFIXES if n >= 64]
    return out
