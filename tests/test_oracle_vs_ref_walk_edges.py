"""CPU: the restatement against the reference's own render.cl compiled for x86-64 at signed-zero directions -- cameras with a
zeroed row of either sign and with fov_scale = 0 (tests/bvh_walk_cases.py ref_check_cameras). As tests/test_oracle_vs_ref.py:
bit-identical to that build's stored outputs (tests/golden/walk_edges_ref.npz, tests/golden/make_golden.py --walk-edges), and,
where oracle/_ref is built, to the live build as well. The GPU tests of the walk's edges lean on the oracle at these cameras."""
import numpy as np
import pytest

import bvh_walk_cases as W
from conftest import bits_equal
from golden_io import GOLDEN


@pytest.fixture(scope="module")
def cameras():
    return W.ref_check_cameras()


@pytest.fixture(scope="module")
def stored():
    z = np.load(GOLDEN / "walk_edges_ref.npz")
    return {k: z[k] for k in z.files if k != "detmath_revision"}


def test_the_cameras_are_the_degenerate_ones(stored, cameras):
    assert sorted(stored) == sorted(f"frame/{n}" for n in cameras) and len(cameras) >= 12
    signs, fov0 = set(), 0
    for rec in cameras.values():
        _, dirs = W.primary_rays(rec)
        signs |= {"-" if s else "+" for s in np.signbit(dirs[dirs == 0])}
        fov0 += rec["fov"] == 0.0
        rows = rec["cam"][:3, :3]
        signs |= {"row-" for a in range(3) if (rows[:, a] == 0).all() and np.signbit(rows[:2, a]).all()}
        signs |= {"row+" for a in range(3) if (rows[:, a] == 0).all() and not np.signbit(rows[:2, a]).any()}
    assert signs == {"+", "-", "row+", "row-"} and fov0 >= 6


@pytest.mark.parametrize("name", sorted(W.REF_CHECK_NAMES))
def test_signed_zero_cameras(name, cameras, oracle, ref, stored, sky):
    a = W.render_with(oracle, cameras[name], sky)
    assert bits_equal(a, stored[f"frame/{name}"]), f"{name}: port differs from the reference build's stored output"
    if ref is not None:
        assert bits_equal(a, W.render_with(ref, cameras[name], sky)), f"{name}: port differs from the live reference build"
