"""The nearest-surface walk's pruning, pinned on the CPU (no device): tests/nearest_walk_ref.py restates the walk of
csrc/device_nearest.h in numpy float32; here it is compared with the contract (tests/nearest_ref.py's brute force) word for word
on the directed families of tests/nearest_walk_cases.py and a fixed-seed random set, every box it left out is audited against
the triangles beneath it, its stack is measured against the host's bound, deliberately wrong walks are shown to be told apart by
a named family each, and the generators are shown to reach what they claim. tests/test_gpu_nearest_walk_edges.py runs the same
families on the device."""
import functools

import numpy as np
import pytest

import nearest_ref as NR
import nearest_walk_cases as NC
import nearest_walk_ref as NW
from simple_raytracer_amd import records as R, tracer as T

F = np.float32
N_RANDOM = 100  # per mesh and tree, beside the directed families (about 1,000 queries): what keeps this module near a minute
MESH_TREES = [(n, k) for n in NC.MESHES for k in NC.TREES]

# which family of which mesh and tree tells each wrong walk apart from the contract (test_a_wrong_walk_is_caught)
CAUGHT_BY = {
    "no_slack": ("grid", "sah", "far_query"),
    "prune_at_equal": ("squares_underflow", "sah", "near_surface"),
    "key_rounds_up": ("squares_underflow", "sah", "far_query"),
    "tie_first_visited": ("grid", "sah", "tie_across_leaves"),
    "model_gate_relative": ("blob968_far", "sah", "tangent_ball"),
}


@functools.lru_cache(maxsize=None)
def outcome(name, kind):
    """the restatement's records and logs, the brute force's records and the audit of one mesh and tree over the directed
    families and the random set; computed once"""
    sc = NC.scene(name)
    pts, md, fam = NC.directed(name, kind)
    rp, rm = NC.random_queries(name, kind, N_RANDOM)
    pts, md, fam = np.concatenate([pts, rp]), np.concatenate([md, rm]), np.concatenate([fam, np.full(len(rp), "random")])
    qs = R.point_queries(pts, md)
    got, logs = NW.run(sc["shapes"], sc["tris"], NC.tree(name, kind), qs, log=True)
    want = NR.brute_force(sc["shapes"], sc["tris"], qs)
    return dict(qs=qs, fam=fam, got=got, want=want, logs=logs, audit=NW.audit(sc["shapes"], sc["tris"], NC.tree(name, kind), qs, got, logs))


@pytest.mark.parametrize("name,kind", MESH_TREES)
def test_restatement_equals_the_brute_force(name, kind):
    o = outcome(name, kind)
    bad = np.nonzero((NR.words(o["got"]) != NR.words(o["want"])).any(1))[0]
    assert not len(bad), (len(bad), sorted(set(o["fam"][bad].tolist())), o["qs"][bad[0]], o["got"][bad[0]], o["want"][bad[0]])
    for fam in NC.FAMILIES:
        if fam == "tie_across_leaves" and name not in ("grid", "grid_far", "two_models"):
            continue
        if fam == "tangent_ball" and name == "squares_underflow":  # (every d2 and every distance is 0 there: no ball to size)
            continue
        if fam == "inside_overlap" and not NC.overlap_points(name, kind):  # (a tree of a few triangles may have no two children that overlap)
            continue
        assert (o["fam"] == fam).any(), fam


@pytest.mark.parametrize("name,kind", MESH_TREES)
def test_no_box_left_out_holds_the_answer(name, kind):
    """soundness, exact: no skipped box (gate, child, popped entry) holds a triangle whose computed distance is below the
    record's, or equal to it with a lower index; and the rounding has used less of the slack than the slack has"""
    a = outcome(name, kind)["audit"]
    print(f"nearest walk audit {name:18s} {kind:6s}: {a['boxes']:7d} boxes left out, largest undercut {a['undercut']:8.2f} of {NW.SLACK_UNITS} units; "
          f"over every box tested {a['undercut_any']:6.2f}")
    assert not a["unsound"], a["unsound"][:4]
    assert a["undercut"] < NW.SLACK_UNITS
    # a box that was entered could have been left out under another best: the slack must cover its undercut as well
    assert a["undercut_any"] < NW.SLACK_UNITS


@pytest.mark.parametrize("name,kind", MESH_TREES)
def test_stack_stays_within_the_hosts_bound(name, kind):
    o = outcome(name, kind)
    for i, m in NC.tree(name, kind).items():
        assert m["stack_need"] <= T.BVH_STACK_CAP
        assert o["logs"][i]["deepest"].max() <= m["stack_need"], (i, int(o["logs"][i]["deepest"].max()), m["stack_need"])
    deep = o["fam"] == "deepest_stack"
    assert deep.sum() == 4 and max(o["logs"][i]["deepest"][deep].max() for i in o["logs"]) == max(o["logs"][i]["deepest"].max() for i in o["logs"])


def _run(name, kind, fam, wrong):
    sc = NC.scene(name)
    pts, md = NC.family(name, kind, fam)
    qs = R.point_queries(pts, md)
    got, logs = NW.run(sc["shapes"], sc["tris"], NC.tree(name, kind), qs, wrong=wrong, log=True)
    return got, NR.brute_force(sc["shapes"], sc["tris"], qs), sum(len(lg["tested"]) for lg in logs.values())


@pytest.mark.parametrize("wrong", sorted(CAUGHT_BY))
def test_a_wrong_walk_is_caught(wrong):
    name, kind, fam = CAUGHT_BY[wrong]
    got, want, _ = _run(name, kind, fam, wrong)
    assert (NR.words(got) != NR.words(want)).any(), (wrong, name, kind, fam)
    right, _, _ = _run(name, kind, fam, None)
    assert np.array_equal(NR.words(right), NR.words(want))


@pytest.mark.parametrize("name,kind", [("grid", "sah"), ("blob968", "median"), ("slivers", "sah"), ("tiny_13", "median"), ("two_models", "sah")])
def test_not_retesting_a_popped_entry_is_harmless(name, kind):
    """no_retest_shrinks: the re-test of a popped entry only saves work -- the same records, more triangles tested"""
    for fam in ("near_surface", "on_child_plane"):
        got, want, tested = _run(name, kind, fam, "no_retest_shrinks")
        assert np.array_equal(NR.words(got), NR.words(want))
        assert tested > _run(name, kind, fam, None)[2]


# ---- the generators reach what they claim -------------------------------------------------------------------------------------------
def test_tiny_trees_have_the_shapes_they_are_there_for():
    leaf_roots, nks, cnts = 0, set(), set()
    for k in NC.TINY:
        for kind in NC.TREES:
            sc = NC.scene(f"tiny_{k}")
            wide, _ = NC.host_tree(sc["shapes"][0], sc["tris"], kind)
            m = NC.tree(f"tiny_{k}", kind)[0]
            leaf_roots += bool(wide["root"] & T.BVH_LEAF_BIT)
            nks |= {int(m["nk"][i]) for i in m["inner"]}
            cnts |= {(tag >> 2) & 3 for i in m["inner"] for _, tag in m["children"][i] if tag & 16} | ({(wide["root"] >> 28) & 3} if wide["root"] & T.BVH_LEAF_BIT else set())
    assert leaf_roots >= 1 and {2, 3, 4} <= nks and {1, 2, 3} <= cnts, (leaf_roots, nks, cnts)


@pytest.mark.parametrize("name,kind", [("grid", "sah"), ("grid_far", "median"), ("blob968", "sah"), ("slivers", "median"), ("mixed_scale_far", "sah"), ("tiny_7", "sah")])
def test_plane_points_are_on_their_planes(name, kind):
    trees = NC.tree(name, kind)
    seen = set()
    for i, idx, k, axis, side, what, p in NC.plane_points(name, kind):
        m = trees[i]
        plane = (m["lo"], m["hi"])[side][axis] if idx < 0 else NC.decoded(m, idx)[side][k][axis]
        if what == "on":  # bitwise on the plane. The gate's lo - q is then a zero; a child's fmaf(byte, 2^e, origin - q) rounds
            # origin - q first and may come out an ulp of the coordinate off zero: both sides of "on" are cases of their own
            assert p[axis].view(np.uint32) == plane.view(np.uint32)
            d = (NW.gate_d2(m, p[None])[0] if idx < 0 else NW.children_d2(m, idx, p[None])[:, k])[0]
            assert d == 0 if idx < 0 else d <= (np.float64(np.spacing(max(abs(p[axis]), abs(m["origin"][idx][axis])))) * 2) ** 2
            assert (m["lo"] if idx < 0 else NC.decoded(m, idx)[0][k])[(axis + 1) % 3] < p[(axis + 1) % 3]
        elif what in ("below", "above"):
            assert p[axis] == np.nextafter(plane, F(-np.inf if what == "below" else np.inf))
            d = (NW.gate_d2(m, p[None])[0] if idx < 0 else NW.children_d2(m, idx, p[None])[:, k])[0]
        else:
            lo, hi = (m["lo"], m["hi"]) if idx < 0 else [b[k] for b in NC.decoded(m, idx)]
            assert all(p[a].view(np.uint32) in (lo[a].view(np.uint32), hi[a].view(np.uint32)) for a in range(3))
        seen.add((axis, side, what, bool(np.signbit(p[axis]))))
    assert {(a, s, w) for a, s, w, _ in seen} == {(a, s, w) for a in range(3) for s in (0, 1) for w in ("on", "below", "above", "corner")}
    if name in ("grid", "blob968", "slivers"):
        assert {(a, neg) for a, _, w, neg in seen if w == "on"} == {(a, neg) for a in range(3) for neg in (False, True)}


@pytest.mark.parametrize("name,kind", [("grid", "sah"), ("grid", "median"), ("blob968", "sah"), ("slivers", "median"), ("tiny_13", "sah")])
def test_overlap_points_lie_in_several_children_with_keys_of_zero(name, kind):
    trees = NC.tree(name, kind)
    pts = NC.overlap_points(name, kind)
    assert len(pts) >= 4
    for i, idx, inside, p in pts:
        assert len(inside) >= 2
        assert not NW.children_d2(trees[i], idx, p[None])[0][inside].view(np.uint32).any()  # +0: the keys are the tags alone


@pytest.mark.parametrize("name,kind", [("grid", "sah"), ("blob968", "median"), ("mixed_scale_far", "sah")])
def test_tangent_balls_touch_their_boxes(name, kind):
    m = NC.tree(name, kind)[0]
    t = NC.tangent_points(name, kind)
    assert {x[0] for x in t} == {"gate", "child"}
    for n in range(0, len(t), 3):
        what, p, _, d2 = t[n]
        slack = NW.gate_d2(m, p[None])[1]
        r2 = [NW.reach2(np.asarray([t[n + j][2]], F), slack)[0] for j in range(3)]
        assert r2[0] < d2 <= r2[1] <= r2[2] and t[n + 1][2] == np.nextafter(t[n][2], F(np.inf))  # the first float whose ball reaches the box
    exact = sum(NW.reach2(np.asarray([x[2]], F), NW.gate_d2(m, x[1][None])[1])[0] == x[3] for x in t)
    assert exact >= 1, "no ball's reach2 equals its box's d2 bit for bit"


@pytest.mark.parametrize("name", ["grid", "grid_far", "two_models"])
def test_ties_really_tie_across_leaves_in_both_orders(name):
    sc = NC.scene(name)
    ties = NC.tie_points(name)
    pts = np.asarray([p for _, p, _ in ties], F)
    orders = set()
    for kind in NC.TREES:
        trees = NC.tree(name, kind)
        got, logs = NC.run_ref(name, kind, pts, np.full(len(pts), np.inf, F), log=True)
        assert np.array_equal(got["distance"].astype(np.float64), [h for _, _, h in ties])  # the exact distance, in float64
        tied_in_all = np.zeros(len(pts), np.int64)
        for i, m in trees.items():
            d = NR.triangle(m["wrec"][None, :, :], pts[:, None, :])[0]
            tied = d == got["distance"][:, None]
            tied_in_all += tied.sum(1)
            slot_of = {int(t): s for s, t in enumerate(m["slot_tri"]) if t >= 0}
            first_seen = {}
            for qi, slot, trip in logs[i]["tested"]:
                first_seen.setdefault((int(qi), int(slot)), len(first_seen))
            for qi in range(len(pts)):
                tris = np.nonzero(tied[qi])[0]
                leaves = {slot_of[int(t)] >> 2 for t in tris}
                seen = sorted((first_seen[(qi, slot_of[int(t)])], int(t)) for t in tris if (qi, slot_of[int(t)]) in first_seen)
                if len(leaves) >= 2 and len(seen) >= 2:
                    orders.add(seen[0][1] < seen[1][1])
        assert (tied_in_all >= 2).all()
        if name == "two_models":
            assert (got["shape"] == 0).all()  # the second model's coinciding triangle ties; strict-less keeps the first
            d1 = NR.triangle(trees[1]["wrec"][None, :, :], pts[:, None, :])[0].min(1)
            assert (d1 >= got["distance"]).all() and (d1 == got["distance"]).sum() >= len(pts) // 2  # (its sheet across x has moved off)
    assert orders == {True, False}, orders


def test_squares_underflow_to_zero():
    """the mesh of 2^-80: every d2 and every reach2 after the first leaf is +0, where > and >= part"""
    m = NC.tree("squares_underflow", "sah")[0]
    pts, md = NC.family("squares_underflow", "sah", "near_surface")
    r0, _ = NW.root_entry(m["root"])
    assert not NW.children_d2(m, r0, pts).any() and not NW.gate_d2(m, pts)[0].any()
    got = NC.run_ref("squares_underflow", "sah", pts, md)[0]
    assert not NW.reach2(got["distance"], NW.gate_d2(m, pts)[1]).any()


def test_far_queries_overflow():
    for name in ("grid", "slivers"):
        m = NC.tree(name, "sah")[0]
        pts, md = NC.family(name, "sah", "far_query")
        d2, slack = NW.gate_d2(m, pts)
        assert np.isinf(d2).sum() == 6 and (NW.max_abs(pts) > 1e3 * m["bmax"]).sum() >= 32
