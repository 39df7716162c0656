"""CPU: the directed cases of tests/bvh_walk_cases.py bite, and the numpy restatement of the walk survives them. Over every
case's pixel-centre rays: each triangle that the ray really hits (Moller-Trumbore in float64 from the float32 ray) is among
those the float32 walk tests; the walk ends within the hierarchy's bounds. The cases reach what they aim at: every axis sees
a +0 and a -0 direction component (hence both signs of the safe inverse at a zero), every mesh and tree has a ray whose entry
distance before the clamp is -0.0 at a child that leads to a hit, and a walk that is wrong in the clamp or in the sign of the
safe inverse loses a hit on these rays -- shown by running those wrong walks here."""
import numpy as np
import pytest

import bvh_walk_cases as W

MESH_TREES = [(m, k) for m in W.MESH_NAMES for k in W.TREES]
MINUS_ZERO = 0x80000000


def lost(rec, org, d, wrong=None, events=None):
    """the triangles that the ray hits and the walk never tested"""
    sc, tr = W.scene(rec["mesh"]), W.tree(rec["mesh"], rec["tree"])
    tested, steps, deepest = W.walk(tr["wide"], tr["tri_of_slot"], org, d, wrong=wrong, events=events, fields=tr["fields"])
    assert steps <= len(tr["wide"]["blocks"]) and deepest <= tr["wide"]["stack_need"], rec["name"]
    hits = W.true_hits(sc["wv"], org.astype(np.float64), d.astype(np.float64))
    return set(hits.tolist()) - set(tested), len(hits)


_frames = {}


def frame(rec):
    """per ray of the case: (triangles lost, triangles hit), once per case"""
    if rec["name"] not in _frames:
        org, dirs = W.primary_rays(rec)
        _frames[rec["name"]] = [lost(rec, org, d) for d in dirs]
    return _frames[rec["name"]]


def test_case_counts():
    """what DESIGN.md section 5 states, and what the GPU test's run time rests on"""
    counts = {fam: len(W.all_cases(fam)) for fam in W.FAMILIES}
    print(counts)
    assert counts == {"on_plane_in": 198, "on_plane_out": 198, "on_plane_along": 396, "one_ulp": 396, "axis_parallel": 342, "in_plane_grazing": 144}
    for rec in W.all_cases():
        assert rec["w"] * rec["h"] <= 16 * 8 and rec["spp"] in (1, 2) and rec["bounces"] in (1, 2)
    names = [rec["name"] for rec in W.all_cases()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("mesh,kind", MESH_TREES)
def test_origins_lie_on_decoded_planes_of_every_level_child_axis_and_side(mesh, kind):
    tr = W.tree(mesh, kind)
    origins = W.plane_origins(mesh, kind)
    level_of = {idx: lv for lv, idxs in enumerate(tr["levels"]) for idx in idxs}
    assert len(tr["levels"]) >= 3
    assert {level_of[o[0]] for o in origins} == set(range(len(tr["levels"])))
    assert {o[1] for o in origins} == {0, 1, 2, 3} and {(o[2], o[3]) for o in origins} == {(a, s) for a in range(3) for s in (0, 1)}
    for idx, k, axis, side, org in origins:
        first, nk, tags, los, his = W.inner_children(tr["wide"]["blocks"], idx)
        assert org[axis].tobytes() == (los[k], his[k])[side][axis].tobytes()
        assert all(los[k][b] < org[b] < his[k][b] for b in range(3) if b != axis)
    cases = W.cases(mesh, kind)
    planes = [(level_of[o[0]], o[1], o[2], o[3]) for o in origins]
    for fam, per_origin in (("on_plane_in", 1), ("on_plane_out", 1), ("on_plane_along", 2), ("one_ulp", 2)):  # the same origins, all of them
        assert [(level_of[r["block"]], r["child"], r["axis"], r["side"]) for r in cases[fam]] == [p for p in planes for _ in range(per_origin)], fam
        for n, rec in enumerate(cases[fam]):
            org, moved = origins[n // per_origin][4], rec["cam"][3, :3]
            if fam == "one_ulp":
                assert abs(int(moved[rec["axis"]].view(np.int32)) - int(org[rec["axis"]].view(np.int32))) == 1
                moved = np.where(np.arange(3) == rec["axis"], org, moved)
            assert moved.tobytes() == org.tobytes(), rec["name"]
    assert {r["zero_sign"] for r in cases["on_plane_along"]} == {"+", "-"}


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("mesh,kind", MESH_TREES)
def test_the_oracle_subset_is_spread_and_mixed(mesh, kind, family):
    """the frames that the GPU test also holds to the CPU oracle: first and last record of the family (the root's level and the
    deepest), show_normals and path-traced frames, both bounce counts and both sample counts"""
    recs = W.cases(mesh, kind)[family]
    if not recs:
        return
    sub = W.oracle_subset(mesh, kind, family, 10)
    assert len(sub) == 10 and sub[0] is recs[0] and sub[-1] is recs[-1]
    assert {r["show_normals"] for r in sub} == {True, False} and {r["bounces"] for r in sub} == {1, 2} and {r["spp"] for r in sub} == {1, 2}
    assert sum(not r["show_normals"] for r in sub) >= 5


@pytest.mark.parametrize("mesh,kind", [(m, k) for m, k in MESH_TREES if m != "blob968"])
def test_equal_distance_hits_sit_in_different_leaves(mesh, kind):
    """axis_parallel over a vertex, an edge's midpoint and a diagonal's: the ray hits several triangles of one sheet at one t, and
    in most of these cases they lie in different leaf blocks, so the lower-index rule has to hold across leaves"""
    tr, sc = W.tree(mesh, kind), W.scene(mesh)
    leaf_of = {tri: slot >> 2 for slot, tri in tr["tri_of_slot"].items()}
    spots = [r for r in W.cases(mesh, kind)["axis_parallel"] if r.get("spot") in ("vertex", "edge", "diagonal")]
    tied = across = 0
    for rec in spots:
        org, dirs = W.primary_rays(rec)
        hits = W.true_hits(sc["wv"], org.astype(np.float64), dirs[0].astype(np.float64))
        if len(hits) >= 2:
            tied += 1
            across += len({leaf_of[int(t)] for t in hits}) >= 2
    print(len(spots), tied, across)
    assert len(spots) == 30 and tied >= 24 and 2 * across >= tied


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("mesh,kind", MESH_TREES)
def test_every_truly_hit_triangle_is_tested(mesh, kind, family):
    n_hits = 0
    for rec in W.cases(mesh, kind)[family]:
        for ray, (missing, hits) in enumerate(frame(rec)):
            assert not missing, f"{rec['name']} ray {ray}: triangles {sorted(missing)} are hit but were never tested"
            n_hits += hits
    assert n_hits > 0 or not W.cases(mesh, kind)[family]


@pytest.mark.parametrize("family", ["on_plane_in", "axis_parallel"])
@pytest.mark.parametrize("mesh,kind", MESH_TREES)
def test_at_least_half_of_the_cases_hit_the_model(mesh, kind, family):
    """what tests/test_gpu_bvh_walk_edges.py asserts of the device's frames: here by at least two pixel centres per case, so a
    jittered sample cannot undo it"""
    recs = W.cases(mesh, kind)[family]
    hit = sum(1 for rec in recs if sum(1 for _, hits in frame(rec) if hits) >= 2)
    assert 2 * hit >= len(recs), (hit, len(recs))


def zero_signs(family=None):
    """per axis the set of signs ('+', '-') of the exactly zero direction components over the cases' restated rays"""
    seen = [set(), set(), set()]
    for rec in W.all_cases(family):
        _, dirs = W.primary_rays(rec)
        for a in range(3):
            z = dirs[:, a] == 0
            seen[a] |= {"-" if s else "+" for s in np.signbit(dirs[z, a])}
    return seen


def test_every_axis_sees_both_zeros_and_both_signs_of_the_safe_inverse():
    """(the safe inverse of a zero is copysign(2^100, zero): a +0 and a -0 component are its two signs)"""
    assert zero_signs() == [{"+", "-"}] * 3
    for fam in ("axis_parallel", "on_plane_along", "in_plane_grazing"):  # each of the families built for it, on its own
        assert zero_signs(fam) == [{"+", "-"}] * 3, fam


@pytest.mark.parametrize("mesh,kind", MESH_TREES)
def test_minus_zero_before_the_clamp_on_the_path_to_a_hit_and_the_wrong_clamp_loses_it(mesh, kind):
    """on_plane_in from a hi plane: the child the origin lies on has an entry distance of -0.0 before the clamp and is entered,
    and the walk whose clamp keeps that sign never tests a triangle below that child which the ray hits"""
    found = None
    for rec in W.cases(mesh, kind)["on_plane_in"]:
        org, dirs = W.primary_rays(rec)
        for ray, d in enumerate(dirs):
            if frame(rec)[ray][1] == 0:
                continue
            events = []
            missing, _ = lost(rec, org, d, events=events)
            assert not missing
            if not any(bits == MINUS_ZERO and entered for _, _, bits, entered in events):
                continue
            wrong_missing, _ = lost(rec, org, d, wrong="clamp_sign")
            if wrong_missing:
                found = (rec["name"], ray, sorted(wrong_missing))
                break
        if found:
            break
    print(found)
    assert found, "no on_plane_in ray has -0.0 before the clamp at a child that leads to a hit"


def test_a_safe_inverse_without_the_zeros_sign_loses_hits():
    """axis_parallel and on_plane_along: with +2^100 for a -0 component under planes chosen for a negative direction, a box the
    ray runs through looks missed. Taking -0 for +0 in BOTH places is no error (the same ray; padded boxes hold no triangle in
    their own planes), and loses nothing on any case."""
    losing = {fam: 0 for fam in ("axis_parallel", "on_plane_along")}
    for fam in losing:
        for rec in W.all_cases(fam):
            org, dirs = W.primary_rays(rec)
            for ray, d in enumerate(dirs):
                if frame(rec)[ray][1] == 0 or not (np.signbit(d) & (d == 0)).any():
                    continue
                assert not lost(rec, org, d, wrong="zero_sign_folded")[0], (rec["name"], ray)
                if lost(rec, org, d, wrong="inverse_sign")[0]:
                    losing[fam] += 1
    print(losing)
    assert all(n > 0 for n in losing.values()), losing
