"""CPU: the restatement must be bit-identical to the reference's own render.cl compiled for x86-64 -- to that build's
outputs stored in tests/golden/ref_checks.npz (tests/golden/make_golden.py --ref-checks), and, where oracle/_ref is
built, to the live build as well."""
import numpy as np
import pytest

import cases as C
import golden_io
from conftest import bits_equal

FRAMES = C.ref_check_frames()


@pytest.fixture(scope="module")
def stored():
    return golden_io.load_ref_checks()


def _check_frame(name, oracle, ref, stored, sky):
    a = C.render_frame(oracle, FRAMES[name], sky)
    assert bits_equal(a, stored[f"frame/{name}"]), f"{name}: port differs from the reference build's stored output"
    if ref is not None:
        assert bits_equal(a, C.render_frame(ref, FRAMES[name], sky)), f"{name}: port differs from the live reference build"


def test_sphere_scene_config0_slice(oracle, ref, stored, sky):
    _check_frame("sphere_slab", oracle, ref, stored, sky)


def test_mesh_scene(oracle, ref, stored, sky):
    _check_frame("mesh", oracle, ref, stored, sky)


def test_random_time_seeds(oracle, ref, stored, sky):
    names = [n for n in FRAMES if n.startswith("seed_")]
    assert len(names) == 4
    for name in names:
        _check_frame(name, oracle, ref, stored, sky)


def test_average_bytes(oracle, ref, stored, sky):
    _check_frame("average_input", oracle, ref, stored, sky)
    a = C.average_input(stored["frame/average_input"])  # the reference build's frame (tests/golden/make_golden.py resolves the same)
    for steps in C.AVERAGE_STEPS:
        got = oracle.average(steps, a)
        assert np.array_equal(got, stored[f"average/{steps}"]), steps
        if ref is not None:
            assert np.array_equal(got, ref.average(steps, a)), steps
