"""What the deformed-refit tests share (tests/test_bvh_deform_host.py, tests/test_gpu_bvh_deform.py): the models of
tests/bvh_refit_cases.py deformed -- a smooth wave of 5 % of the model's diagonal, a scramble that throws every vertex to a
point of its own in the model's box, a wave that leaves a NaN vertex behind, an axis flattened -- and the host's cost
ratios of the two deformations the rebuild rule is tested with. A plain module, not a test module."""
import functools

import numpy as np

import bvh_refit_cases as K
from simple_raytracer_amd import records as R, tracer as T

F = np.float32
SIZES = ["n1", "n3", "n4", "n7", "n200", "n6k"]


def base(model):
    return R.as_records(K.model_triangles(model), R.TRIANGLE)


def _box(tris):
    p = np.asarray(tris["v"]["pos"], np.float64)[..., :3].reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def wave(tris, step=1, amplitude=0.05):
    """every vertex position + a * sin(k . p + phase) per axis, a = amplitude x the model's diagonal (5 %); the normals stay.
    `step` moves the phase: another step, another mesh."""
    out = tris.copy()
    lo, hi = _box(tris)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    a = amplitude * diag
    p = np.asarray(tris["v"]["pos"], np.float64)[..., :3]
    kvec = np.array([[2.1, 0.7, -1.3], [-0.9, 1.9, 0.8], [1.1, -1.4, 2.3]]) * (2.0 * np.pi / max(diag, 1e-30))
    phase = np.array([0.3, 1.1, 2.0]) + 0.37 * step
    d = a * np.sin(p @ kvec.T + phase)
    out["v"]["pos"][..., :3] = (p + d).astype(F)
    return out


def scramble(tris, seed=5):
    """every vertex to an independent uniform point of the model's box: the case that wrecks the tree"""
    out = tris.copy()
    lo, hi = _box(tris)
    rng = np.random.default_rng(seed)
    shape = np.asarray(tris["v"]["pos"])[..., :3].shape
    out["v"]["pos"][..., :3] = (lo + (hi - lo) * rng.random(shape)).astype(F)
    return out


def with_nan(tris):
    """the wave, and one vertex of a triangle in the middle NaN, one of another inf"""
    out = wave(tris, step=3)
    out["v"]["pos"][len(out) // 2, 1, 0] = np.nan
    if len(out) > 2:
        out["v"]["pos"][len(out) // 3, 2, 1] = np.inf
    return out


def flattened(tris):
    """the wave with every y the same: extent 0 on one axis"""
    out = wave(tris, step=2)
    out["v"]["pos"][..., 1] = F(0.25)
    return out


def shape_over(tris, transform=None, material=0, first=0, count=None):
    with np.errstate(all="ignore"):
        return R.model(material, tris, first, len(tris) - first if count is None else count, R.identity4() if transform is None else transform)


@functools.lru_cache(maxsize=None)
def ratios(model):
    """(wave's cost ratio, scramble's) of the host, hierarchy built over the base mesh at the identity"""
    t0 = base(model)
    out = []
    for now in (wave(t0), scramble(t0)):
        built, cost = T.bvh_wide_cost_host(shape_over(t0), t0, shape_over(now), now)
        out.append(cost / built)
    return tuple(out)
