"""CPU: the per-shape motion table of the temporal stage's object motion (srt_motion_table_host, host only) against its
float64 formulas (tests/motion_ref.py), the numpy restatement of the moved set-up kernel (tests/temporal_ref.py reproject
with a table) on analytic cases, its agreement with the path without a table, and the flagged share of the moves
tests/test_gpu_denoise_motion.py runs."""
import numpy as np
import pytest

import motion_ref as M
import temporal_ref as TR
from gpu_harness import cam_at, scene
from simple_raytracer_amd import records as R, scenes as S, tracer as T
from temporal_cases import geometry_frame
from test_temporal_reference import frame_of, history_of, rd

F32 = np.float32


def one_scene(shape):
    shapes = np.zeros(1, R.SHAPE)  # (zeros first: a record's padding is not copied with it)
    shapes[0] = shape
    return shapes, R.box_triangles(), S.sphere_scene_materials(), R.scene_data(1)


def host_row(hist_shape, cur_shape):
    h, c = one_scene(hist_shape), one_scene(cur_shape)
    return T.motion_table_host(h, c)


def ulps(a, b):
    """distance in float32 ulps of b (float64 values rounded to float32) from a (float32)"""
    a = np.asarray(a, F32)
    want = np.asarray(b, np.float64).astype(F32)
    return np.abs(a.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-45)


def random_affine(rng):
    m = np.eye(4)
    m[:3, :3] = (M.rot_axis(rng.normal(size=3), rng.uniform(-3, 3))[:3, :3] @ np.diag(rng.uniform(0.4, 2.5, 3)) @
                 (np.eye(3) + np.triu(rng.uniform(-0.4, 0.4, (3, 3)), 1)))  # rotation, non-uniform scale, shear
    m[3, :3] = rng.uniform(-5, 5, 3)
    return m.astype(F32)


def random_pair(rng, kind):
    if kind == M.SPHERE:
        return (R.sphere(1, rng.uniform(-5, 5, 3), rng.uniform(0.2, 3)), R.sphere(1, rng.uniform(-5, 5, 3), rng.uniform(0.2, 3)))
    if kind == M.PLANE:
        return (R.plane(1, rng.uniform(-5, 5, 3), rng.normal(size=3) * rng.uniform(0.5, 2)), R.plane(1, rng.uniform(-5, 5, 3), rng.normal(size=3) * rng.uniform(0.5, 2)))
    tris = R.box_triangles()
    return R.model(1, tris, 0, 12, random_affine(rng)), R.model(1, tris, 0, 12, random_affine(rng))


def forward(hist, cur, X):
    """history -> current of the table in include/srt_abi.h, float64, written out independently of the inverse"""
    kind = int(cur["type"])
    if kind == M.SPHERE:
        ph, pc = np.float64(hist["sphere_position"][:3]), np.float64(cur["sphere_position"][:3])
        return pc + (float(cur["sphere_radius"]) / float(hist["sphere_radius"])) * (X - ph)
    if kind == M.PLANE:
        u, v = np.float64(hist["plane_normal"][:3]), np.float64(cur["plane_normal"][:3])
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        k, c = np.cross(u, v), u @ v
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rm = np.eye(3) + K + K @ K / (1 + c)
        assert np.allclose(Rm @ u, v, atol=1e-12)
        return np.float64(cur["plane_position"][:3]) + (X - np.float64(hist["plane_position"][:3])) @ Rm.T
    mh, mc = np.float64(hist["transform"]).T, np.float64(cur["transform"]).T  # math 4x4
    G = mc @ np.linalg.inv(mh)
    return X @ G[:3, :3].T + G[:3, 3]


# ---- 1. the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [M.SPHERE, M.PLANE, M.MODEL])
def test_table_matches_float64_formulas_and_inverts_the_move(kind):
    rng = np.random.RandomState(10 + kind)
    for _ in range(40):
        hist, cur = random_pair(rng, kind)
        got = host_row(hist, cur)
        state, A, B = M.table_row(hist, cur)
        assert got is not None and got["state"][0] == state == M.MOVED
        assert ulps(got["A"][0], A).max() <= 1 and ulps(got["B"][0], B).max() <= 1
        X = rng.uniform(-4, 4, (16, 3))
        Xc = forward(hist, cur, X)
        back = Xc @ np.float64(got["A"][0][:, :3]).T + np.float64(got["A"][0][:, 3])
        # A is float32: each of its 12 entries is off by at most 2^-24 relative, times the magnitudes it multiplies
        scale = np.abs(Xc) @ np.abs(np.float64(got["A"][0][:, :3])).T + np.abs(np.float64(got["A"][0][:, 3]))
        assert np.all(np.abs(back - X) <= 4 * 2.0 ** -24 * scale + 1e-12)
        L = forward(hist, cur, np.eye(3)) - forward(hist, cur, np.zeros((1, 3)))  # rows: L e_k -> L^T
        assert np.allclose(got["B"][0], L, rtol=1e-6, atol=1e-6)  # B = L^T


def test_identical_records_are_static_and_no_history_cases():
    tris = R.box_triangles()
    for s in (R.sphere(1, (1, 2, 3), 0.5), R.plane(1, (0, 1, 0), (0, 2, 0)), R.model(1, tris, 0, 12, R.translate((1, 2, 3)))):
        got = host_row(s, s)  # (two arrays with the same bytes)
        assert got["state"][0] == M.STATIC and np.array_equal(got["A"][0], np.eye(3, 4)) and np.array_equal(got["B"][0], np.eye(3))
    sing = R.model(1, tris, 0, 12, R.scale_matrix((1, 0, 1)))
    nan_m = R.model(1, tris, 0, 12, R.translate((np.nan, 0, 0)))
    good = R.model(1, tris, 0, 12, R.translate((1, 0, 0)))
    cases = [(R.sphere(1, (0, 0, 0), r0), R.sphere(1, (1, 0, 0), r1)) for r0, r1 in ((0, 1), (1, 0), (-1, 1), (1, -2), (np.inf, 1), (1, np.nan))]
    cases += [(R.plane(1, (0, 0, 0), (0, 0, 0)), R.plane(1, (0, 1, 0), (0, 1, 0))), (R.plane(1, (0, 0, 0), (0, 1, 0)), R.plane(1, (0, 1, 0), (0, 0, 0))),
              (R.plane(1, (0, 0, 0), (0, 1, 0)), R.plane(1, (0, 0, 0), (0, -3, 0)))]  # a zero normal; the opposite normal (c = -1)
    cases += [(sing, good), (good, sing), (nan_m, good), (good, nan_m)]
    for hist, cur in cases:
        got = host_row(hist, cur)
        assert got is not None and got["state"][0] == M.NO_HISTORY == M.table_row(hist, cur)[0], (hist, cur)


def test_edits_outside_the_allowed_fields_drop():
    shapes, tris, mats = S.mixed_test_scene()
    sd = R.scene_data(len(shapes))
    base = (shapes, tris, mats, sd)
    assert np.all(T.motion_table_host(base, base)["state"] == M.STATIC)
    moved = M.move_shapes(shapes, tris, M.MOVES[-1][4], 1)
    got, want = T.motion_table_host(base, (moved, tris, mats, sd)), M.scene_table(base, (moved, tris, mats, sd))
    assert got["state"].tolist() == want["state"].tolist() == [0, 1, 0, 0, 1, 0, 0, 1]
    assert ulps(got["A"], want["A"]).max() <= 1 and ulps(got["B"], want["B"]).max() <= 1

    def edit(field, idx, value):
        s = shapes.copy()
        s[field][idx] = value
        return (s, tris, mats, sd)

    t2, m2, sd2 = tris.copy(), mats.copy(), sd.copy()
    t2["v"]["pos"][20, 0, 0] += 0.5
    m2[0]["smoothness"] = 0.5
    sd2["sun_intensity"] = 2.0
    as_plane = shapes.copy()
    as_plane[1] = R.plane(2, (0, 0, 0), (0, 1, 0))
    drops = [edit("material", 1, 3), edit("triangle_index", 3, 1), edit("num_triangles", 4, 100), (shapes[:-1], tris, mats, sd),
             (np.concatenate([shapes, shapes[:1]]), tris, mats, sd), (as_plane, tris, mats, sd), (shapes, t2, mats, sd), (shapes, tris[:-1], mats, sd),
             (shapes, tris, m2, sd), (shapes, tris, mats[:-1], sd), (shapes, tris, mats, sd2)]
    for i, cur in enumerate(drops):
        assert T.motion_table_host(base, cur) is None and M.scene_table(base, cur) is None, i


# ---- 2. the kernel's restatement on analytic cases ---------------------------------------------------------------------
def quad_frame(w, h, L, cam_rd, x_lo, x_hi, ids_value=1):
    """a camera-facing quad at z = -L covering x_lo <= x < x_hi (world), in front of nothing: Z, cov, ids"""
    c0, c1, c2, cam, aspect, fov = TR.camera(cam_rd)
    ys, xs = np.mgrid[0:h, 0:w]
    sx = ((2 * (xs + 0.5) / w - 1) * aspect) * fov
    sy = (1 - 2 * (ys + 0.5) / h) * fov
    d = np.stack([sx, sy, -np.ones_like(sx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    Z = ((cam[2] + L) / -d[..., 2]).astype(F32)
    X = cam[0] + Z * d[..., 0]
    on = (X >= x_lo) & (X < x_hi)
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1
    c = np.random.RandomState(4).uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    f = frame_of(c, N, np.where(on, Z, 0).astype(F32), cov=on.astype(F32))
    return f, np.where(on, ids_value, M.NO_SHAPE).astype(np.uint32)


def table_for(A, B=None, n=2, idx=1):
    t = M.static_table(n)
    t["state"][idx] = M.MOVED
    t["A"][idx] = np.asarray(A, np.float64).astype(F32)
    t["B"][idx] = np.eye(3, dtype=F32) if B is None else np.asarray(B, np.float64).astype(F32)
    return t


def test_translated_quad_finds_its_history_k_pixels_back():
    w, h, L = 64, 36, 4.0
    cam = rd(w, h, R.camera_matrix((0.0, 0.0, 0.0)))
    pix = 2.0 * (w / h) * L / w
    for k in (1, 3, -2):
        hist_f, hist_ids = quad_frame(w, h, L, cam, -1.0, 1.0)
        cur_f, ids = quad_frame(w, h, L, cam, -1.0 + k * pix, 1.0 + k * pix)
        A = np.hstack([np.eye(3), [[-k * pix], [0], [0]]])  # current -> history: back by k pixel widths
        fx, fy, Dist, front = TR.project(cur_f["Z"], cam, cam, w, h, A=np.broadcast_to(A.astype(F32), (h, w, 3, 4)))
        on = ids == 1
        xs = np.broadcast_to(np.arange(w)[None, :], (h, w))
        assert on.any() and np.abs(fx - (xs - k))[on].max() < 2e-3 and np.abs(fy - np.arange(h)[:, None])[on].max() < 2e-3
        hist = history_of(hist_f, hist_f["c"], 6.0, cam)
        hist["guide"][..., 1, 3] = hist_f["cov"]
        hist["ids"] = hist_ids
        rep = TR.reproject(cur_f, hist, cam, ids=ids, table=table_for(A))
        inner = on & (hist_ids[:, np.clip(np.arange(w) - k, 0, w - 1)] == 1)
        assert np.all(rep["h"][inner & ~rep["borderline"]] > 0) and np.all(rep["h"][~on] == 0)
        src = hist["colour"][:, np.clip(np.arange(w) - k, 0, w - 1)]
        sel = inner & (rep["taps"] == 4)
        assert sel.any() and np.allclose(rep["c"][sel], src[sel], rtol=2e-2, atol=2e-2)
        # the same pixels without the map look at where the quad was not: the shape index rejects what they find there
        wrong = dict(hist, ids=np.where(hist_ids == 1, 0, hist_ids).astype(np.uint32))
        assert np.all(TR.reproject(cur_f, wrong, cam, ids=ids, table=table_for(A))["h"] == 0)


def test_scaled_sphere_maps_a_hit_to_the_same_angle():
    w, h = 48, 48
    cam = rd(w, h, R.camera_matrix((0.0, 0.0, 5.0)))
    centre, r_h, r_c = np.array([0.3, -0.2, -1.0]), 1.0, 1.3
    hist_s, cur_s = R.sphere(1, centre, r_h), R.sphere(1, centre, r_c)
    state, A, B = M.table_row(hist_s, cur_s)
    centre, r_c = np.float64(hist_s["sphere_position"][:3]), float(cur_s["sphere_radius"])  # the records' float32 values
    rng = np.random.RandomState(2)
    dirs = rng.normal(size=(50, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    Xc = centre + r_c * dirs
    Xh = Xc @ A[:, :3].T + A[:, 3]
    assert state == M.MOVED and np.allclose(Xh, centre + r_h * dirs, atol=1e-12)
    nh = dirs @ B.T
    assert np.allclose(nh / np.linalg.norm(nh, axis=1, keepdims=True), dirs, atol=1e-12)


def test_nothing_moved_equals_temporal_ref_bit_for_bit():
    w, h = 40, 24
    rng = np.random.RandomState(6)
    N = rng.normal(size=(h, w, 3)).astype(F32)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    cur = frame_of(rng.uniform(0, 3, (h, w, 3)), N, rng.uniform(3, 6, (h, w)))
    ids = rng.randint(0, 3, (h, w)).astype(np.uint32)
    for cam_h in (R.camera_matrix((0.0, 0.5, 5.0), 0.3, -0.1), R.camera_matrix((0.02, 0.5, 5.0), 0.31, -0.1)):
        cam_rd, cam_h_rd = rd(w, h, R.camera_matrix((0.0, 0.5, 5.0), 0.3, -0.1)), rd(w, h, cam_h)
        hist = history_of(cur, rng.uniform(0, 3, (h, w, 3)), 5.0, cam_h_rd)
        hist["ids"] = ids
        want = TR.reproject(cur, hist, cam_rd)
        got = TR.reproject(cur, hist, cam_rd, ids=ids, table=M.static_table(3))  # the moved kernel's path with every shape static
        for k in ("h", "c", "m1", "m2", "taps", "borderline"):
            assert np.array_equal(got[k], want[k]), k
        assert (want["h"] > 0).any()
        # a history pixel that showed a shape which has since moved does not count for a static pixel
        t = M.static_table(3)
        t["state"][2] = M.MOVED
        got = TR.reproject(cur, hist, cam_rd, ids=np.zeros((h, w), np.uint32), table=t)
        assert np.all(got["taps"] <= want["taps"]) and (got["taps"] < want["taps"]).any()


# ---- 3. moving everything rigidly = moving the history camera the other way -----------------------------------------------
def test_rigid_move_of_every_shape_equals_moving_the_history_camera():
    w, h = 64, 36
    rng = np.random.RandomState(9)
    cam_m = R.camera_matrix((0.3, 0.5, 5.0), 0.2, -0.1)
    cam_rd = rd(w, h, cam_m)
    Z = rng.uniform(3, 9, (h, w)).astype(F32)
    for _ in range(5):
        G = M.rot_axis(rng.normal(size=3), rng.uniform(-0.05, 0.05))  # history -> current, column layout
        G[3, :3] = rng.uniform(-0.1, 0.1, 3)
        Gm = G.T  # math
        Ainv = np.linalg.inv(Gm)[:3, :]  # current -> history
        cam_h_m = (np.float64(cam_m) @ G).astype(F32)  # column layout: (G C)^T = C^T G^T
        cam_h_rd = rd(w, h, cam_h_m)
        a = TR.project(Z, cam_rd, cam_rd, w, h, A=np.broadcast_to(Ainv.astype(F32), (h, w, 3, 4)))
        b = TR.project(Z, cam_rd, cam_h_rd, w, h)
        truth = TR.project(Z, cam_rd, cam_h_rd, w, h, dtype=np.float64)
        assert a[3].all() and b[3].all()
        # float32 rounding of either route: the point and both camera positions are at most `mag` from the origin, ~10
        # rounded operations lead to the view vector v (each within 2^-24 of a value <= ~3 mag: the 3-term sums), q = v.xy / -v.z
        # carries (|dv| + |q| |dv|) / |v.z|, and f = q W / (2 aspect fov). The inputs differ too: A, the moved camera and the
        # host's inverse are rounded to float32 (2^-24 each, times mag). D carries |dv| alone.
        eps = 2.0 ** -24
        mag = float(np.abs(np.float64(cam_m[3, :3])).max() + Z.max() + np.abs(G[3, :3]).max())
        dv = 16 * eps * 3 * mag
        vz = float(truth[2].min()) * 0.5  # |v.z| >= D cos(half field of view); fov_scale 1, aspect 16 / 9: cos >= 0.44
        qmax = float(cam_rd["aspect_ratio"] * cam_rd["fov_scale"]) * 1.2
        tol_f = (dv * (1 + qmax) / vz) * w / (2 * float(cam_rd["aspect_ratio"] * cam_rd["fov_scale"]))
        for route in (a, b):
            assert np.abs(route[0] - truth[0]).max() <= tol_f and np.abs(route[1] - truth[1]).max() <= tol_f
            assert np.abs(route[2] - truth[2]).max() <= dv
        assert tol_f < 1e-2  # the bound itself is far below a pixel


# ---- 6 (CPU part). the flagged share of the GPU test's moves ---------------------------------------------------------
@pytest.mark.parametrize("case", M.MOVES, ids=[m[0] for m in M.MOVES])
def test_moves_stay_under_the_flagged_share(oracle, case):
    """at most 1 % of a frame's pixels flagged, for every move of the GPU test; the moved shape has pixels with history and
    disoccluded pixels without"""
    FRAMES, SIZE = M.FRAMES, M.SIZE
    name, scn, accel, cam_kind, steps = case
    w, h = SIZE
    shapes, tris, mats = scene(scn)
    sd = R.scene_data(len(shapes))
    prev = None
    for k in range(FRAMES):
        now = M.move_shapes(shapes, tris, steps, k)
        cur, ids, rdata = geometry_frame(oracle, scn, cam_at(k, cam_kind), now, tris, mats, w, h, 2000 + k)
        if prev is not None:
            p_cur, p_ids, p_rd, p_shapes = prev
            table = M.scene_table((p_shapes, tris, mats, sd), (now, tris, mats, sd))
            assert table is not None and [i for i, s in enumerate(table["state"]) if s == M.MOVED] == sorted(s[0] for s in steps)
            hist = TR.history_from_commit(TR.integrate(p_cur, TR.reproject(p_cur, dict(valid=False), p_rd))["commit"], p_rd)
            hist["ids"] = p_ids
            rep = TR.reproject(cur, hist, rdata, ids=ids, table=table)
            share = rep["borderline"].mean()
            on_moved = np.isin(ids, [s[0] for s in steps])
            kept, lost = on_moved & (rep["h"] > 0), (cur["cov"] > 0) & (rep["taps"] == 0) & ~rep["borderline"]
            print(f"{name} frame {k}: flagged {share * 100:.3f}%, moved-shape pixels with history {kept.sum()}, without any {lost.sum()}")
            assert share <= 0.01, (name, k, share)
            assert kept.any() and lost.any(), (name, k)
        prev = (cur, ids, rdata, now)
