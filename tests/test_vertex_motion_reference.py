"""CPU: per-triangle motion of the temporal stage (srt_set_denoise_vertex_motion). The keep rule and the table of
srt_motion_table_deform_host (host only) against tests/vertex_motion_ref.py, srt_motion_table_host unchanged beside it, the
per-pixel map of a deformed triangle pinned analytically, and the flagged share of the deformations
tests/test_gpu_denoise_vertex_motion.py runs."""
import numpy as np
import pytest

import motion_ref as M
import temporal_ref as TR
import vertex_motion_ref as V
from simple_raytracer_amd import records as R, scenes as S, tracer as T
from temporal_cases import geometry_frame

F32 = np.float32


def base_scene():
    shapes, tris, mats = S.mesh_scene()  # a plane and two instances over one range of 968 triangles (12 box triangles before it)
    return shapes, tris, mats, R.scene_data(len(shapes))


def two_models():
    shapes, tris, mats = S.mixed_test_scene()  # models 2, 3 (box), 4 (smooth, 12..212), 6 (flat, 212..308)
    return shapes, tris, mats, R.scene_data(len(shapes))


def same_table(got, want):
    assert got is not None and want is not None
    assert got["state"].tolist() == want["state"].tolist()
    d = want["state"] == V.DEFORMED
    assert got["first_row"][d].tolist() == want["first_row"][d].tolist()
    raw_a, raw_b = got["A"].view(np.uint32).reshape(len(d), -1), got["B"].view(np.uint32).reshape(len(d), -1)
    assert np.all(raw_a[d][:, 1:] == 0) and np.all(raw_b[d] == 0)  # a DEFORMED row: state, first row, zeros
    assert np.array_equal(got["A"][~d], want["A"][~d]) or np.abs(got["A"][~d] - want["A"][~d]).max() < 1e-6
    assert np.array_equal(got["B"][~d], want["B"][~d]) or np.abs(got["B"][~d] - want["B"][~d]).max() < 1e-6


# ---- 1. the keep rule and the table ---------------------------------------------------------------------------------------
def test_one_changed_vertex_of_one_model_of_two():
    shapes, tris, mats, sd = two_models()
    t2 = V.copy_tris(tris)
    t2["v"]["pos"][12 + 20, 0, 0] += 0.5  # inside the smooth mesh's range alone
    base, cur = (shapes, tris, mats, sd), (shapes, t2, mats, sd)
    got, want = T.motion_table_host(base, cur, deform=True), V.scene_table(base, cur)
    same_table(got, want)
    assert got["state"].tolist() == [0, 0, 0, 0, V.DEFORMED, 0, 0, 0]
    assert got["first_row"][4] == 24  # behind the two box instances' 12 rows each


def test_two_instances_over_one_range_are_both_deformed():
    shapes, tris, mats, sd = base_scene()
    t2 = V.wave(tris, 12, 968, 1)
    got, want = T.motion_table_host((shapes, tris, mats, sd), (shapes, t2, mats, sd), deform=True), V.scene_table((shapes, tris, mats, sd), (shapes, t2, mats, sd))
    same_table(got, want)
    assert got["state"].tolist() == [0, V.DEFORMED, V.DEFORMED] and got["first_row"][1:].tolist() == [0, 968]


def test_a_deformed_model_that_also_moved_is_deformed():
    shapes, tris, mats, sd = two_models()
    t2 = V.copy_tris(tris)
    t2["v"]["pos"][12 + 3, 1, 1] -= 0.25
    moved = M.move_shapes(shapes, tris, [(4, "translate", (0.1, 0.0, 0.2)), (6, "rotate", 0.1)], 1)
    base, cur = (shapes, tris, mats, sd), (moved, t2, mats, sd)
    got = T.motion_table_host(base, cur, deform=True)
    same_table(got, V.scene_table(base, cur))
    assert got["state"][4] == V.DEFORMED and got["state"][6] == M.MOVED


def test_bytes_outside_every_range_are_not_compared():
    shapes, tris, mats, sd = base_scene()  # the 12 box triangles belong to no model of this scene
    t2 = V.copy_tris(tris)
    t2["v"]["pos"][3, 2, 1] += 1.0
    got = T.motion_table_host((shapes, tris, mats, sd), (shapes, t2, mats, sd), deform=True)
    same_table(got, V.scene_table((shapes, tris, mats, sd), (shapes, t2, mats, sd)))
    assert np.all(got["state"] == M.STATIC)


def test_count_and_range_changes_drop():
    shapes, tris, mats, sd = two_models()
    base = (shapes, tris, mats, sd)

    def edit(field, idx, value):
        s = M.move_shapes(shapes, tris, [], 0)
        s[field][idx] = value
        return (s, tris, mats, sd)

    m2 = mats.copy()
    m2[0]["smoothness"] = 0.5
    drops = [(shapes, tris[:-1], mats, sd), (shapes, np.concatenate([tris, tris[:1]]), mats, sd), edit("num_triangles", 4, 100), edit("triangle_index", 3, 1),
             edit("material", 1, 3), (shapes[:-1], tris, mats, sd), (shapes, tris, m2, sd)]
    for i, cur in enumerate(drops):
        assert T.motion_table_host(base, cur, deform=True) is None and V.scene_table(base, cur) is None, i


def test_identical_ranges_give_the_rows_of_the_plain_table_bit_for_bit():
    shapes, tris, mats, sd = two_models()
    moved = M.move_shapes(shapes, tris, M.MOVES[-1][4], 1)
    flat = M.move_shapes(moved, tris, [], 0)
    flat["sphere_radius"][5] = 0.0  # NO_HISTORY
    for cur_shapes in (shapes, moved, flat):
        plain = T.motion_table_host((shapes, tris, mats, sd), (cur_shapes, tris, mats, sd))
        deform = T.motion_table_host((shapes, tris, mats, sd), (cur_shapes, tris, mats, sd), deform=True)
        for k in ("state", "A", "B"):
            assert np.array_equal(np.ascontiguousarray(plain[k]).view(np.uint8), np.ascontiguousarray(deform[k]).view(np.uint8)), k
    # with one range deformed the other shapes' rows still are
    t2 = V.copy_tris(tris)
    t2["v"]["pos"][12, 0, 0] += 0.1
    deform = T.motion_table_host((shapes, tris, mats, sd), (moved, t2, mats, sd), deform=True)
    plain = T.motion_table_host((shapes, tris, mats, sd), (moved, tris, mats, sd))
    keep = deform["state"] != V.DEFORMED
    assert keep.sum() == len(shapes) - 1
    for k in ("state", "A", "B"):
        assert np.array_equal(np.ascontiguousarray(plain[k][keep]).view(np.uint8), np.ascontiguousarray(deform[k][keep]).view(np.uint8)), k


def test_plain_table_still_drops_on_a_changed_vertex():
    shapes, tris, mats, sd = two_models()
    t2 = V.copy_tris(tris)
    t2["v"]["pos"][12 + 20, 0, 0] += 0.5
    assert T.motion_table_host((shapes, tris, mats, sd), (shapes, t2, mats, sd)) is None
    assert M.scene_table((shapes, tris, mats, sd), (shapes, t2, mats, sd)) is None


def test_world_rows_layout():
    shapes, tris, mats, sd = two_models()
    rows = V.world_rows(shapes, tris)
    first, n = V.first_rows(shapes)
    assert n == len(rows) == 12 + 12 + 200 + 96 and first.tolist() == [0, 0, 0, 12, 24, 224, 224, 320]
    m = np.float64(shapes[4]["transform"]).T
    p = np.float64(tris["v"]["pos"][12 + 7, 2, :3])
    assert np.allclose(rows[24 + 7, 2], m[:3, :3] @ p + m[:3, 3], rtol=1e-6, atol=1e-6)


# ---- 2. the per-pixel map, analytically -----------------------------------------------------------------------------------
def random_triangles(rng, n):
    P = rng.uniform(-3, 3, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    return P.astype(F32)


def test_rigid_motion_of_the_vertices_equals_the_rigid_map():
    """X_h and N_h against applying the rigid map directly (float64). The bound, from the magnitudes of the float64 result:
    every input is within 2^-24 relative of a value of magnitude <= mag (the vertices, X), the differences e, f, d are sums
    of two such (2 eps mag absolute), the Gram entries and right-hand sides are 3-term dot products of them, and the 2x2
    solve amplifies a relative error by its condition a11 a22 / det = 1 / sin^2 of the corner's angle; u, v multiply edges of
    length <= edge. So |X_h - R X - t| <= K eps mag cond with K = 64 covering the ~20 rounded operations, and the unit normal
    carries K eps cond (mag / edge): the vertices' rounding tilts the triangle's plane by eps mag / edge."""
    rng = np.random.RandomState(21)
    eps = 2.0 ** -24
    n = 400
    P = random_triangles(rng, n)
    for _ in range(4):
        G = M.rot_axis(rng.normal(size=3), rng.uniform(-2, 2))[:3, :3].T  # math rotation
        tr = rng.uniform(-2, 2, 3)
        Q = (np.float64(P) @ G.T + tr).astype(F32)  # the history's vertices: the rigid map of the current ones, rounded
        uv = rng.uniform(-0.2, 1.2, (n, 2))  # places inside and a little outside the triangle (not clamped)
        X64 = np.float64(P[:, 0]) + uv[:, :1] * (np.float64(P[:, 1]) - np.float64(P[:, 0])) + uv[:, 1:] * (np.float64(P[:, 2]) - np.float64(P[:, 0]))
        N64 = rng.normal(size=(n, 3))
        N64 /= np.linalg.norm(N64, axis=1, keepdims=True)
        Xh, Nh, ok = V.deform_map(P, Q, X64.astype(F32), N64.astype(F32))
        assert ok.all()
        e1, e2 = np.float64(P[:, 1]) - np.float64(P[:, 0]), np.float64(P[:, 2]) - np.float64(P[:, 0])
        a11, a22, a12 = np.sum(e1 * e1, 1), np.sum(e2 * e2, 1), np.sum(e1 * e2, 1)
        cond = a11 * a22 / (a11 * a22 - a12 * a12)
        mag = np.abs(np.concatenate([np.float64(P).reshape(n, -1), np.float64(Q).reshape(n, -1)], 1)).max(1)
        edge = np.sqrt(np.minimum(a11, a22))
        want_x = X64 @ G.T + tr
        want_n = N64 @ G.T
        assert np.all(np.abs(Xh - want_x).max(1) <= 64 * eps * mag * cond)
        assert np.all(np.abs(Nh - want_n).max(1) <= 64 * eps * cond * np.maximum(mag / edge, 1.0))
        # and the float32 route agrees with the same formulas in float64 within the same bound
        Xd, Nd, okd = V.deform_map(P, Q, X64.astype(F32), N64.astype(F32), dtype=np.float64)
        assert okd.all() and np.all(np.abs(Xh - Xd).max(1) <= 64 * eps * mag * cond)


def test_pure_stretch_of_a_flat_triangle_keeps_the_flat_normal():
    rng = np.random.RandomState(22)
    P = random_triangles(rng, 200)
    S3 = np.diag([1.7, 0.6, 1.2]) @ M.rot_axis((1, 2, 3), 0.4)[:3, :3]
    Q = (np.float64(P) @ S3.T).astype(F32)
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    gc = np.cross(np.float64(e1), np.float64(e2))
    gc /= np.linalg.norm(gc, axis=1, keepdims=True)
    gh = np.cross(np.float64(Q[:, 1]) - np.float64(Q[:, 0]), np.float64(Q[:, 2]) - np.float64(Q[:, 0]))
    gh /= np.linalg.norm(gh, axis=1, keepdims=True)
    for sign in (1.0, -1.0):  # the flat normal, front or back face
        _, Nh, ok = V.deform_map(P, Q, P[:, 0], (sign * gc).astype(F32))
        assert ok.all() and np.abs(Nh - sign * gh).max() < 1e-4


def test_degenerate_triangles_and_nan_give_no_history():
    P = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F32)
    X, N = np.array([[0.2, 0.2, 0.0]], F32), np.array([[0, 0, 1]], F32)
    line = np.array([[[0, 0, 0], [1, 0, 0], [2, 0, 0]]], F32)
    point = np.zeros((1, 3, 3), F32)
    nan = P.copy()
    nan[0, 1, 1] = np.nan
    inf = P.copy()
    inf[0, 2, 0] = np.inf
    assert V.deform_map(P, P, X, N)[2].all()
    for bad in (line, point, nan, inf):
        assert not V.deform_map(bad, P, X, N)[2].any()  # a degenerate current triangle
        assert not V.deform_map(P, bad, X, N)[2].any()  # a degenerate history triangle


def test_deformed_pixels_reproject_through_their_triangles():
    """one camera-facing quad of two triangles at z = -4 that was 1.5 times as wide in the history frame: a pixel on it
    finds its history at the stretched place, and a static pixel rejects a tap that showed the deformed shape"""
    from test_temporal_reference import frame_of, history_of, rd
    w, h, L = 64, 36, 4.0
    cam = rd(w, h, R.camera_matrix((0.0, 0.0, 0.0)))
    Pq = np.array([[[-1, -3, -L], [1, -3, -L], [1, 3, -L]], [[-1, -3, -L], [1, 3, -L], [-1, 3, -L]]], F32)
    Qq = Pq.copy()
    Qq[..., 0] = F32(1.5) * Pq[..., 0]
    Qq[..., 1] = F32(1.1) * Pq[..., 1]  # (and 1.1 times as high: no tap coordinate on a whole pixel)
    X = V.first_hit(np.full((h, w), 1.0, F32), cam, w, h)
    Z = (L / -X[..., 2]).astype(F32)
    X = V.first_hit(Z, cam, w, h)
    on = (np.abs(X[..., 0]) < 1.0) & (np.abs(X[..., 1]) < 3.0)
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1
    colour = np.random.RandomState(5).uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    cur = frame_of(colour, N, Z)
    ids = np.where(on, 1, 0).astype(np.uint32)
    tri = V.nearest_triangles(Pq, np.zeros(3), X.reshape(-1, 3)).reshape(h, w)
    tri_ids = np.where(on, tri, V.NO_TRIANGLE).astype(np.uint32)
    hX = X[..., 0]
    hist = history_of(cur, colour, 6.0, cam)
    hist["ids"] = np.where((hX > -1.5) & (hX < 1.5) & (np.abs(X[..., 1]) < 3.3), 1, 0).astype(np.uint32)  # the history's quad: x in (-1.5, 1.5)
    table = M.static_table(2)
    table["state"][1] = V.DEFORMED
    table["A"][1], table["B"][1] = 0, 0
    table["first_row"] = np.array([0, 0])
    rep = V.reproject(cur, hist, cam, ids=ids, table=table, tri_ids=tri_ids, rows=Pq, h_rows=Qq)
    Xh, _, ok = V.deform_map(Pq[np.where(on, tri, 0)], Qq[np.where(on, tri, 0)], X, N)
    want_x = 1.5 * np.float64(X[..., 0])  # the affine map of the plane: x -> 1.5 x on both triangles (they share the diagonal)
    assert ok[on].all() and np.abs(Xh[..., 0] - want_x)[on].max() < 1e-5
    inner = on & ~rep["borderline"]
    assert inner.any() and np.all(rep["h"][inner] > 0)
    # static pixels beside the quad whose history showed the (then wider) quad: no history; farther out: kept
    was_quad = ~on & (hist["ids"] == 1)
    assert was_quad.any() and np.all(rep["h"][was_quad] == 0)
    far = ~on & (hist["ids"] == 0)
    assert far.any() and np.all(rep["h"][far] == 6.0)
    # a pixel without a triangle index, or one past the model's triangles, has no history
    none = V.reproject(cur, hist, cam, ids=ids, table=table, tri_ids=np.full((h, w), V.NO_TRIANGLE, np.uint32), rows=Pq, h_rows=Qq)
    past = V.reproject(cur, hist, cam, ids=ids, table=table, tri_ids=np.full((h, w), 2, np.uint32), rows=Pq, h_rows=Qq)
    assert np.all(none["h"][on] == 0) and np.all(past["h"][on] == 0) and np.all(none["h"][far] == 6.0)


def test_nothing_deformed_equals_the_moved_restatement_bit_for_bit():
    from test_temporal_reference import frame_of, history_of, rd
    w, h = 40, 24
    rng = np.random.RandomState(6)
    N = rng.normal(size=(h, w, 3)).astype(F32)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    cur = frame_of(rng.uniform(0, 3, (h, w, 3)), N, rng.uniform(3, 6, (h, w)))
    ids = rng.randint(0, 3, (h, w)).astype(np.uint32)
    cam_rd, cam_h_rd = rd(w, h, R.camera_matrix((0.0, 0.5, 5.0), 0.3, -0.1)), rd(w, h, R.camera_matrix((0.02, 0.5, 5.0), 0.31, -0.1))
    hist = history_of(cur, rng.uniform(0, 3, (h, w, 3)), 5.0, cam_h_rd)
    hist["ids"] = ids
    table = M.static_table(3)
    table["state"][2] = M.MOVED
    table["A"][2, 0, 3] = 0.01
    table["first_row"] = np.zeros(3, np.int64)
    want = TR.reproject(cur, hist, cam_rd, ids=ids, table=table)
    got = V.reproject(cur, hist, cam_rd, ids=ids, table=table, tri_ids=np.zeros((h, w), np.uint32), rows=np.zeros((0, 3, 3), F32), h_rows=np.zeros((0, 3, 3), F32))
    for k in ("h", "c", "m1", "m2", "taps", "borderline"):
        assert np.array_equal(got[k], want[k]), k
    assert (want["h"] > 0).any()


# ---- 3. the flagged share of the GPU test's deformations ------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in V.CASES if not c[3]], ids=[c[0] for c in V.CASES if not c[3]])
def test_deformations_stay_under_the_flagged_share(oracle, case):
    """at most 1 % of a frame's pixels flagged by the restatement alone, for every deformation of the GPU test (the device
    upkeep cases deform as mesh-wave does); the deformed models have pixels with history"""
    name, scn, accel, upkeep, cam_kind, deform, steps = case
    w, h = V.SIZE
    shapes, tris, mats = V.case_scene(scn)
    sd = R.scene_data(len(shapes))
    prev = None
    for k in range(V.FRAMES):
        now, now_tris = V.case_frame(case, shapes, tris, k)
        cam_m = V.case_camera(scn, k, cam_kind)
        cur, ids, rdata = geometry_frame(oracle, scn, cam_m, now, now_tris, mats, w, h, 2000 + k)
        rows = V.world_rows(now, now_tris)
        first, _ = V.first_rows(now)
        X = V.first_hit(cur["Z"], rdata, w, h)
        cam = np.float64(TR.camera(rdata)[3])
        tri_ids = np.full((h, w), V.NO_TRIANGLE, np.uint32)
        for s in np.unique(ids[ids != M.NO_SHAPE]):
            if int(now[s]["type"]) != M.MODEL:
                continue
            sel = ids == s
            d = np.float64(X[sel]) - cam
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            best = V.nearest_triangles(rows[first[s]:first[s] + int(now[s]["num_triangles"])], cam, d)
            tri_ids[sel] = np.where(best >= 0, best, V.NO_TRIANGLE).astype(np.uint32)
        if prev is not None:
            p_cur, p_ids, p_rd, p_shapes, p_tris, p_rows = prev
            table = V.scene_table((p_shapes, p_tris, mats, sd), (now, now_tris, mats, sd))
            assert table is not None and (table["state"] == V.DEFORMED).any()
            hist = TR.history_from_commit(TR.integrate(p_cur, TR.reproject(p_cur, dict(valid=False), p_rd))["commit"], p_rd)
            hist["ids"] = p_ids
            rep = V.reproject(cur, hist, rdata, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=p_rows)
            share = rep["borderline"].mean()
            on = rep["state"] == V.DEFORMED
            kept = on & (rep["h"] > 0)
            print(f"{name} frame {k}: flagged {share * 100:.3f}%, deformed pixels {on.sum()}, with history {kept.sum()}")
            assert share <= 0.01, (name, k, share)
            assert on.sum() >= 10 and kept.sum() > 0.5 * on.sum(), (name, k)
        prev = (cur, ids, rdata, now, now_tris, rows)
