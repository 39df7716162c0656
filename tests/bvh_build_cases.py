"""What the device-build tests share (tests/test_bvh_morton_host.py, tests/test_gpu_bvh_build.py): the meshes -- the models of
tests/bvh_refit_cases.py, their with_nan and flattened variants of tests/bvh_deform_cases.py, prefixes of n6k at the sort's
sizes, prefixes of the 262,812-triangle n262k around 1,024 << 8, a mesh whose centroids coincide -- and a numpy statement of the Morton code of include/srt_abi.h (SRT_BUILD_DEVICE):
float32 operations in the builder's order, from the raw triangles and a transform alone. A plain module, not a test module."""
import functools

import numpy as np

import bvh_deform_cases as D

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NONFINITE = 0x40000000
TILE = 1024  # csrc/device_types.h SRT_BUILD_TILE: records per workgroup of the sort, four rounds of 256
# a wave (64, 65), a round of the scatter (256, 257), one tile (1024, 1025), two tiles (2048, 2049)
SORT_SIZES = [64, 65, 256, 257, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
BIG = "n262k"  # blob_mesh(363, 363): 262,812 triangles, the q<count> prefixes' mesh
VARIANTS = {"base": lambda t: t, "with_nan": D.with_nan, "flattened": D.flattened}


@functools.lru_cache(maxsize=None)
def mesh(name, variant="base"):
    """name: a model of tests/bvh_refit_cases.py, p<count> = the first <count> triangles of n6k, q<count> = the first <count> of
    n262k, or same<count> = <count> copies of one triangle (every centroid the same)"""
    if name.startswith("same"):
        tris = np.repeat(D.base("n1"), int(name[4:]))
    elif name.startswith("p"):
        tris = D.base("n6k")[:int(name[1:])].copy()
    elif name.startswith("q"):
        tris = D.base(BIG)[:int(name[1:])].copy()
    else:
        tris = D.base(name)
    return VARIANTS[variant](tris)


def _min_std(a, b):  # std::min(a, b): a unless b < a (a NaN in b is dropped, one in a stays)
    return np.where(b < a, b, a)


def _max_std(a, b):
    return np.where(a < b, b, a)


def boxes(shape, tris):
    """(lo, hi, finite): every triangle's unpadded world box as BvhBuilder::load makes it"""
    first, n = int(shape["triangle_index"]), int(shape["num_triangles"])
    m = np.asarray(shape["transform"], F)
    v = np.asarray(tris["v"]["pos"][first:first + n], F)[..., :3]
    with np.errstate(all="ignore"):
        p = ((m[0][None, None, :3] * v[..., 0:1] + m[1][None, None, :3] * v[..., 1:2]) + m[2][None, None, :3] * v[..., 2:3]) + m[3][None, None, :3] * F(1.0)
        p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
        q1, q2 = p0 + (p1 - p0), p0 + (p2 - p0)
        lo = _min_std(_min_std(_min_std(p0, p1), _min_std(p2, q1)), q2)
        hi = _max_std(_max_std(_max_std(p0, p1), _max_std(p2, q1)), q2)
    return lo, hi, (np.isfinite(lo) & np.isfinite(hi)).all(axis=1)


def morton_codes(shape, tris):
    """uint32 per triangle of the model: the definition of include/srt_abi.h, float32, unfused, in its order"""
    lo, hi, finite = boxes(shape, tris)
    n = len(lo)
    codes = np.full(n, NONFINITE, np.uint32)
    if not finite.any():
        return codes
    mlo, mhi = lo[finite].min(axis=0), hi[finite].max(axis=0)
    with np.errstate(all="ignore"):
        c = F(0.5) * lo + F(0.5) * hi
        ext = mhi - mlo
        f = (c - mlo[None, :]) * (F(1024.0) / ext)[None, :]
        q = np.where(f >= F(1023.0), 1023, np.where(f > F(0.0), np.trunc(np.where(np.isfinite(f), f, 0.0)), 0)).astype(np.uint32)
    q = np.where(((ext > 0) & np.isfinite(ext))[None, :], q, 0).astype(np.uint32)
    code = np.zeros(n, np.uint32)
    for i in range(10):
        code |= (((q[:, 0] >> i) & 1) << (3 * i + 2)) | (((q[:, 1] >> i) & 1) << (3 * i + 1)) | (((q[:, 2] >> i) & 1) << (3 * i))
    return np.where(finite, code, NONFINITE).astype(np.uint32)


def morton_order(shape, tris):
    """the triangles by ascending (code, index)"""
    codes = morton_codes(shape, tris)
    return np.lexsort((np.arange(len(codes)), codes)).astype(np.uint32)
