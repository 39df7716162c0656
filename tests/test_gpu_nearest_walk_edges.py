"""The nearest-surface walk on the device at its decision boundaries (csrc/device_nearest.h, csrc/nearest.hip): the directed
families of tests/nearest_walk_cases.py -- queries on decoded child planes and one ulp off them, inside overlapping children,
balls tangent to a box, exact ties across leaves and across two models, points within the slack of a surface, far and
overflowing queries, the deepest stacks -- on needles, slivers, zero-area triangles, mixed scales, trees of one to thirteen
triangles and squared distances that underflow. All 8 words of every record against tests/nearest_ref.py's brute force, under
the array scan and both hierarchies; no record is left out and no tolerance applies. tests/test_nearest_walk_cases.py shows on
the CPU that these families tell deliberately wrong walks apart."""
import numpy as np
import pytest

import nearest_ref as NR
import nearest_walk_cases as NC
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R
from test_gpu_ray_query import handle

pytestmark = pytest.mark.gpu
F = np.float32
ACCELS = ("scan", "sah", "median")  # what ray_query_cases.ACCELS offers for a mesh
LIMIT = 7 * 512

_cases = {}


def cases(name, families=NC.FAMILIES, **kw):
    """(points, max_distance, family of each, the brute force's records) of a mesh: the families built from the SAH tree's planes
    and from the median tree's, one after the other; computed once and never changed"""
    key = (name, families, tuple(sorted(kw.items())))
    if key not in _cases:
        sc = NC.scene(name)
        parts = [NC.family(name, kind, f) + (f,) for kind in NC.TREES for f in families]
        pts, md = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        fam = np.concatenate([np.full(len(p[0]), p[2]) for p in parts])
        assert 0 < len(pts) <= LIMIT
        _cases[key] = (pts, md, fam, NR.brute_force(sc["shapes"], sc["tris"], R.point_queries(pts, md), **kw))
    return _cases[key]


def check(got, want, fam, what):
    bad = np.nonzero((NR.words(got) != NR.words(want)).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} records differ ({sorted(set(fam[bad].tolist()))}), first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


@pytest.mark.parametrize("name,accel", [(n, a) for n in NC.MESHES for a in ACCELS])
def test_every_family_equals_the_brute_force(name, accel, T):
    sc = NC.scene(name)
    pts, md, fam, want = cases(name)
    t = handle(T, (sc["shapes"], sc["tris"], sc["mats"]), accel)
    check(t.nearest_points(pts, md), want, fam, (name, accel))
    assert t.counters()["watchdog"] == 0
    t.close()


@pytest.mark.parametrize("accel", ACCELS)
def test_two_models_without_the_tie_partner(accel, T):
    """every triangle of the second model coincides with one of the first: with either model left out the other answers alone"""
    sc = NC.scene("two_models")
    t = handle(T, (sc["shapes"], sc["tris"], sc["mats"]), accel)
    both = cases("two_models")[3]
    for skip in (0, 1):
        pts, md, fam, want = cases("two_models", skip_shape=skip)
        assert not (want["shape"] == skip).any() and (both["shape"] == skip).any()
        check(t.nearest_points(pts, md, skip_shape=skip), want, fam, ("two_models", accel, "skip", skip))
    assert t.counters()["watchdog"] == 0
    t.close()


@pytest.mark.parametrize("name,kind", [(n, k) for n in ("grid", "grid_far", "blob968") for k in NC.TREES])
def test_ties_and_near_surface_after_a_device_refit(name, kind, T):
    """the model translated by binary fractions (the grids' ties stay exact) and its boxes refitted on the device, not built"""
    sc = NC.scene(name)
    sh, tr, ma = sc["shapes"], sc["tris"], sc["mats"]
    move = np.asarray((0.5, -0.25, 1.0), F)
    pts, md, fam, before = cases(name, ("tie_across_leaves", "near_surface"))
    t = handle(T, (sh, tr, ma), kind, refit=True)
    moved = sh.copy()
    moved[0] = R.model(int(sh["material"][0]), tr, 0, int(sh["num_triangles"][0]), R.mat_mul(R.translate(move), sh["transform"][0]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    pts = (pts + move).astype(F)
    want = NR.brute_force(moved, tr, R.point_queries(pts, md))
    assert ((want["flags"] & R.NEAREST_FOUND) != 0).all()
    if name != "blob968":  # the translation is exact for the grids' binary fractions: the same ties at the same distances
        ties = fam == "tie_across_leaves"
        assert ties.any() and np.array_equal(want["distance"][ties], before["distance"][ties]) and np.array_equal(want["triangle"][ties], before["triangle"][ties])
    check(t.nearest_points(pts, md), want, fam, (name, kind, "refit"))
    assert t.counters()["watchdog"] == 0
    t.close()
