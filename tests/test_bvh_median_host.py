"""CPU: the host statement of the median-split order (include/srt_abi.h SRT_BUILD_ORDER_MEDIAN; no GPU involved). The order
(srt_bvh_median_order_host) against a numpy restatement of the definition (tests/bvh_median_cases.py), up to 262,147 triangles
(nine global levels on the device) against the restatement by depth, itself held to the definition; the hierarchy
(srt_bvh_median_wide_host): the Morton statement's topology with other leaves; its cost against the Morton tree's and the host's
balanced tree's; the setter's validation without a handle; and the two calls on small and hostile meshes under AddressSanitizer
and UndefinedBehaviorSanitizer as a stand-alone program (tests/csrc/bvh_median_check.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bvh_build_cases as B
import bvh_deform_cases as D
import bvh_median_cases as M
from simple_raytracer_amd import tracer as T

ROOT = Path(__file__).resolve().parent.parent
CASES = M.CASES + [("n1", "base"), ("blob968", "base")]
# cost(median) <= (1 + EXCESS) * cost(host balanced): the largest excess measured over M.cost_meshes() is 0.0098 (n200; DESIGN.md
# section 5 has the table), rounded up to the next 0.05. Both trees split the same ranges at the same count on the same axis and
# differ in how the ties of a 16-bit cell fall.
EXCESS = 0.05


def mesh_of(model, variant):
    if model == "blob968":
        name, shape, tris = M.cost_meshes()[2]
        assert name == "mesh968[0]"
        return shape, tris
    tris = B.mesh(model, variant)
    return D.shape_over(tris), tris


@pytest.mark.parametrize("model,variant", CASES)
def test_order_is_the_definitions(model, variant):
    shape, tris = mesh_of(model, variant)
    n = int(shape["num_triangles"])
    got = T.bvh_median_order_host(shape, tris)
    assert np.array_equal(np.sort(got), np.arange(n))  # a permutation
    assert np.array_equal(got, M.median_order(shape, tris))
    if model.startswith("same") or n <= M.LEAF_MAX:
        assert np.array_equal(got, np.arange(n))  # every key is 0 / nothing is split: the identity
    if model == "n6k" and variant == "base":
        assert not np.array_equal(got, np.arange(n)) and not np.array_equal(got, T.bvh_morton_order_host(shape, tris))
    if variant == "with_nan" and n > M.LEAF_MAX:
        finite = B.boxes(shape, tris)[2]
        assert not finite.all() and not finite[got[-1]]  # (behind every finite triangle of every range that is sorted)


@pytest.mark.parametrize("model,variant", CASES)
def test_statement_by_depth_is_the_looped_one(model, variant):
    """M.median_order_by_depth, which the counts past 2^18 are compared with, against the definition's loop over ranges"""
    shape, tris = mesh_of(model, variant)
    assert np.array_equal(M.median_order_by_depth(shape, tris), M.median_order(shape, tris))


@pytest.mark.parametrize("model", M.BIG_CASES)
def test_order_is_the_definitions_at_eight_and_nine_global_levels(model):
    """262,144 triangles: 256 ranges of exactly SRT_BUILD_LOCAL; 262,147: a ninth level. The statement is the one by depth (the
    loop over ranges takes tens of seconds here), held equal to the loop above."""
    shape, tris = mesh_of(model, "base")
    n = int(shape["num_triangles"])
    assert n == int(model[1:]) and M.global_levels(n) == {M.LOCAL << 8: 8, (M.LOCAL << 8) + 3: 9}[n]
    got = T.bvh_median_order_host(shape, tris)
    assert np.array_equal(np.sort(got), np.arange(n))
    assert np.array_equal(got, M.median_order_by_depth(shape, tris))
    assert not np.array_equal(got, np.arange(n))


@pytest.mark.parametrize("model,variant", CASES)
def test_blocks_are_the_morton_statements_topology(model, variant):
    shape, tris = mesh_of(model, variant)
    n = int(shape["num_triangles"])
    got, morton = T.bvh_median_wide_host(shape, tris), T.bvh_morton_wide_host(shape, tris)
    assert got["blocks"].shape == morton["blocks"].shape and got["root"] == morton["root"]
    assert got["stack_need"] == morton["stack_need"] <= 45
    assert np.array_equal(got["dest"], morton["dest"])
    inner = got["blocks"][:, 3] != 0
    assert np.array_equal(inner, morton["blocks"][:, 3] != 0) and not got["blocks"][~inner].any()
    assert np.array_equal(got["blocks"][inner, 10:12], morton["blocks"][inner, 10:12])  # tags and first child: the topology
    if variant == "base" and not model.startswith("same"):
        assert got["cost"] > 0.0


def test_no_triangles():
    tris = B.mesh("n3")
    shape = D.shape_over(tris, count=0)
    got = T.bvh_median_wide_host(shape, tris)
    assert got["root"] == T.BVH_NONE and len(got["blocks"]) == 0 and got["stack_need"] == 0 and got["cost"] == 0.0
    assert len(T.bvh_median_order_host(shape, tris)) == 0


_costs = {}


def costs():
    """name -> (median, Morton, host balanced), once"""
    if not _costs:
        for name, shape, tris in M.cost_meshes():
            balanced, _ = T.bvh_wide_cost_host(shape, tris, shape, tris, force_balanced=True)
            _costs[name] = (T.bvh_median_wide_host(shape, tris)["cost"], T.bvh_morton_wide_host(shape, tris)["cost"], balanced)
    return _costs


@pytest.mark.parametrize("name", ["n200", "n6k", "mesh968[0]", "mesh968[1]"])
def test_cost_is_below_the_morton_trees(name):
    median, morton, balanced = costs()[name]
    print(f"{name}: median {median!r} morton {morton!r} host balanced {balanced!r}")
    assert 0.0 < median < morton


def test_cost_is_the_host_balanced_trees_within_the_margin():
    worst = 0.0
    for name, (median, morton, balanced) in costs().items():
        print(f"{name}: median {median!r} morton {morton!r} host balanced {balanced!r} excess {median / balanced - 1.0:+.4f}")
        worst = max(worst, median / balanced - 1.0)
    print(f"largest excess {worst:.4f}")
    for name, (median, morton, balanced) in costs().items():
        assert 0.0 < median <= (1.0 + EXCESS) * balanced, name


def test_launch_formula():
    """what tests/test_gpu_bvh_build_median.py expects of the counters, at the counts DESIGN.md names"""
    assert [M.global_levels(n) for n in (1, M.LOCAL, M.LOCAL + 1, 2 * M.LOCAL, 2 * M.LOCAL + 1, 4 * M.LOCAL + 3, 6050, 99904)] == [0, 0, 1, 1, 2, 3, 3, 7]
    assert M.launches(M.LOCAL) == 1 and M.launches(M.LOCAL + 1) == 12 and M.launches(6050) == 34 and M.launches(99904) == 78
    # 1,024 << 8: the last count of eight levels, three passes each; three more: a ninth level, of four passes
    assert [M.global_levels(n) for n in M.BIG_PREFIXES] == [8, 9] and M.BIG_PREFIXES == [262144, 262147]
    assert M.launches(262144) == 8 * (2 + 9) + 1 and M.launches(262147) == 8 * (2 + 9) + (2 + 12) + 1


def test_setters_refuse_without_a_handle():
    lib = T.load_library()
    for order in (T.BUILD_ORDER_MORTON, T.BUILD_ORDER_MEDIAN, 2, -1):
        assert lib.srt_set_acceleration_build_order(None, order) == 1  # SRT_ERR_INVALID
        assert lib.srt_group_set_acceleration_build_order(None, order) == 1
    assert lib.srt_bvh_median_order_host(None, None, 0, None, 0) == 1
    assert lib.srt_bvh_median_wide_host(None, None, 0, None, 0, None, 0, None, None, None, None) == 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stand_alone_check_under_sanitizers(tmp_path):
    """tests/csrc/bvh_median_check.cpp with bvh_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program of
    its own: no report, exit status 0."""
    csrc = ROOT / "simple-raytracer_amd" / "csrc"
    exe = tmp_path / "bvh_median_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", f"-I{csrc}", str(ROOT / "tests/csrc/bvh_median_check.cpp"), str(csrc / "bvh_host.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "ok" in r.stdout
