"""CPU: the in-place refit of the wide hierarchy (srt_bvh_refit_wide_host, the host statement of what SRT_REFIT_DEVICE computes
on the device; no GPU involved). The topology the hierarchy was folded with stays; every inner block's byte boxes are
recomputed around the moved triangles -- checked against padded triangle boxes recomputed in numpy from the raw triangles
and the new transform, not against the builder's own boxes. And the builder with the refit under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program (tests/csrc/bvh_refit_check.cpp)."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bvh_refit_cases as K
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
sys.setrecursionlimit(10000)


@pytest.mark.parametrize("balanced", [False, True])
@pytest.mark.parametrize("model", ["n1", "n3", "n4", "n13", "n200", "chain400"])
def test_refit_to_the_same_transform_is_the_built_hierarchy(model, balanced):
    built, _, tris = K.shapes_of(model, "translate")
    wide = T.bvh_wide_host(built, tris, force_balanced=balanced)
    again = T.bvh_refit_wide_host(built, built, tris, force_balanced=balanced)
    assert again["root"] == wide["root"]
    assert np.array_equal(again["blocks"], wide["blocks"])


@pytest.mark.parametrize("balanced", [False, True])
@pytest.mark.parametrize("model,move", K.CASES)
def test_refitted_boxes_contain_the_moved_triangles(model, move, balanced):
    built, moved, tris = K.shapes_of(model, move)
    wide = T.bvh_wide_host(built, tris, force_balanced=balanced)
    order = T.bvh_wide_order_host(built, tris, force_balanced=balanced)
    if not wide["balanced"]:
        assert np.array_equal(order, T.bvh_build_host(built, tris)[1])
    refit = T.bvh_refit_wide_host(built, moved, tris, force_balanced=balanced)
    b0, b1 = wide["blocks"], refit["blocks"]
    # the topology is the built one's: block count, root, and every block's child count, tags and first
    assert b1.shape == b0.shape and refit["root"] == wide["root"]
    assert np.array_equal(b1[:, 3] >> 24, b0[:, 3] >> 24) and np.array_equal(b1[:, 10:], b0[:, 10:])
    lo, hi = K.padded_boxes(moved, tris)
    inner = K.check_contains(b1, refit["root"], wide["dest"], order, lo, hi)
    assert len(inner) == int((b0[:, 3] != 0).sum()) and (len(inner) > 0) == (len(tris) > 3)
    if len(tris) == 6050:
        assert len(inner) > 1024


def test_mismatched_models_are_refused():
    built, moved, tris = K.shapes_of("n13", "rotate")
    other = moved.copy()
    other["num_triangles"] = 12
    with pytest.raises(T.SrtError):
        T.bvh_refit_wide_host(built, other, tris)
    other = moved.copy()
    other["triangle_index"] = 1
    other["num_triangles"] = 12
    b2 = built.copy()
    b2["num_triangles"] = 12
    with pytest.raises(T.SrtError):
        T.bvh_refit_wide_host(b2, other, tris)
    with pytest.raises(T.SrtError):
        T.bvh_refit_wide_host(built, R.sphere(0, (0, 0, 0), 1.0), tris)  # not a model
    assert len(T.bvh_refit_wide_host(b2, b2, tris)["blocks"]) > 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_builder_and_refit_under_sanitizers(tmp_path):
    """tests/csrc/bvh_refit_check.cpp: build, in-place refit and host refit of a few meshes (hostile values included),
    compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer together with bvh_host.cpp, run as a program of its
    own: no report, exit status 0."""
    csrc = ROOT / "simple-raytracer_amd" / "csrc"
    exe = tmp_path / "bvh_refit_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", f"-I{csrc}", str(ROOT / "tests/csrc/bvh_refit_check.cpp"), str(csrc / "bvh_host.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "ok" in r.stdout
