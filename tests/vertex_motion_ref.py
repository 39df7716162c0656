"""Per-triangle motion of the denoiser's temporal stage (include/srt_abi.h srt_set_denoise_vertex_motion,
simple-raytracer_amd/csrc/temporal.hip) in numpy: the keep rule and the table with the DEFORMED state, the world-vertex
rows, the per-pixel map of a deformed triangle, and srt_temporal_kernel<2, ...>'s reprojection -- temporal_ref.reproject with
the deformed branch, branching only where SRT_TEMPORAL_MOTION == 2 does. Everything float32 in the kernel's order, unfused.
"""
import numpy as np

import motion_ref as M
import temporal_ref as TR
from temporal_ref import MOVED, NO_HISTORY, STATIC  # noqa: F401

F32 = np.float32
DEFORMED = 3  # include/srt_abi.h SRT_MOTION_DEFORMED
NO_TRIANGLE = 0xFFFFFFFF


# ---- the keep rule and the table ------------------------------------------------------------------------------------------
def first_rows(shapes):
    """per shape its first row in the vertex tables (model shapes in shape order), and the number of rows"""
    first, rows = np.zeros(len(shapes), np.int64), 0
    for k, s in enumerate(shapes):
        first[k] = rows
        if int(s["type"]) == M.MODEL:
            rows += int(s["num_triangles"])
    return first, rows


def scene_table(hist, cur):
    """motion_ref.scene_table under per-triangle motion: the triangle arrays need only have the same count; a model with a
    differing byte in its range is DEFORMED {state, first_row, zeros}; bytes outside every range are not compared. None =
    the history is dropped, else dict state, A, B (float32) and first_row (n,)."""
    (hs, ht, hm, hd), (cs, ct, cm, cd) = hist, cur
    if len(hs) != len(cs) or len(ht) != len(ct) or hm.tobytes() != cm.tobytes() or np.asarray(hd).tobytes() != np.asarray(cd).tobytes():
        return None
    for a, b in zip(hs, cs):
        if a["type"] != b["type"] or a["material"] != b["material"]:
            return None
        if int(a["type"]) == M.MODEL:
            if a["triangle_index"] != b["triangle_index"] or a["num_triangles"] != b["num_triangles"]:
                return None
            if int(b["triangle_index"]) + int(b["num_triangles"]) > len(ct):
                return None
    first, _ = first_rows(cs)
    eye = (np.zeros((3, 4)), np.zeros((3, 3)))
    rows = []
    for a, b in zip(hs, cs):
        i, n = int(b["triangle_index"]), int(b["num_triangles"])
        if int(a["type"]) == M.MODEL and ht[i:i + n].tobytes() != ct[i:i + n].tobytes():
            rows.append((DEFORMED,) + eye)
        else:
            rows.append(M.table_row(a, b))
    return dict(state=np.array([r[0] for r in rows], np.int64), A=np.array([r[1] for r in rows], np.float64).astype(F32).reshape(-1, 3, 4),
                B=np.array([r[2] for r in rows], np.float64).astype(F32).reshape(-1, 3, 3), first_row=first)


# ---- the world-vertex rows ------------------------------------------------------------------------------------------------
def world_rows(shapes, tris):
    """(rows, 3, 3) float32: P0, P1, P2 of every instance triangle, mat_by_vec(transform, pos, 1.0f) in the pre-pass's
    expressions (frame.hip srt_prepass_kernel), model shapes in shape order"""
    out = []
    for s in shapes:
        if int(s["type"]) != M.MODEL:
            continue
        m = np.asarray(s["transform"], F32)  # m[col][row]
        i, n = int(s["triangle_index"]), int(s["num_triangles"])
        v = np.asarray(tris["v"]["pos"][i:i + n], F32)[..., :3]  # (n, 3 vertices, xyz)
        with np.errstate(all="ignore"):
            w = [((m[0, r] * v[..., 0] + m[1, r] * v[..., 1]) + m[2, r] * v[..., 2]) + m[3, r] * F32(1.0) for r in range(3)]
        out.append(np.stack(w, -1).astype(F32))
    return np.concatenate(out, 0) if out else np.zeros((0, 3, 3), F32)


# ---- the per-pixel map ----------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def deform_map(P, Q, X, N, dtype=F32):
    """P, Q (..., 3, 3): the triangle now and in the history frame; X, N (..., 3): the first hit and the pixel's normal ->
    X_h, N_h (..., 3), ok (...) bool (False: no history). dtype float64 runs the same formulas in double (tests)."""
    P, Q, X, N = (np.asarray(a, dtype) for a in (P, Q, X, N))
    with np.errstate(all="ignore"):
        p0, q0 = P[..., 0, :], Q[..., 0, :]
        e1, e2, f1, f2 = P[..., 1, :] - p0, P[..., 2, :] - p0, Q[..., 1, :] - q0, Q[..., 2, :] - q0
        a11, a12, a22 = dot(e1, e1), dot(e1, e2), dot(e2, e2)
        det = a11 * a22 - a12 * a12
        c, h = cross(e1, e2), cross(f1, f2)
        lc, lh = np.sqrt(dot(c, c)), np.sqrt(dot(h, h))
        ok = (det > 0) & np.isfinite(det) & (lc > 0) & np.isfinite(lc) & (lh > 0) & np.isfinite(lh)
        d = X - p0
        de1, de2 = dot(d, e1), dot(d, e2)
        u, v = (a22 * de1 - a12 * de2) / det, (a11 * de2 - a12 * de1) / det
        Xh = (q0 + u[..., None] * f1) + v[..., None] * f2
        ne1, ne2 = dot(N, e1), dot(N, e2)
        nu, nv = (a22 * ne1 - a12 * ne2) / det, (a11 * ne2 - a12 * ne1) / det
        cn = dot(N, c / lc[..., None])
        t = (nu[..., None] * f1 + nv[..., None] * f2) + cn[..., None] * (h / lh[..., None])
        ln = np.sqrt(dot(t, t))
        ok = ok & (ln > 0) & np.isfinite(ln) & np.all(np.isfinite(Xh), -1)
        Nh = t / ln[..., None]
    return Xh.astype(dtype), Nh.astype(dtype), ok


def first_hit(Z, cam_rd, width, height):
    """X = cam + Z d (h, w, 3) float32, d the camera ray through each pixel's centre: temporal_ref.project's expressions"""
    c0, c1, c2, cam, aspect, fov = TR.camera(cam_rd)
    ys, xs = np.mgrid[0:height, 0:width]
    with np.errstate(all="ignore"):
        ndc_x = (xs.astype(F32) + F32(0.5)) / F32(width)
        ndc_y = (ys.astype(F32) + F32(0.5)) / F32(height)
        sx = ((F32(2) * ndc_x - F32(1)) * aspect) * fov
        sy = (F32(1) - F32(2) * ndc_y) * fov
        r = [((c0[k] * sx + c1[k] * sy) + c2[k] * F32(-1)) + cam[k] * F32(0) for k in range(3)]
        rs = TR.rsqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        Zt = np.asarray(Z, F32)
        return np.stack([cam[k] + Zt * (r[k] * rs) for k in range(3)], -1).astype(F32)


def project_point(X, cam_h_rd, width, height):
    """a world point (h, w, 3) into the history camera: temporal_ref.project behind its map -> fx, fy, D, in_front"""
    rinv = TR.invert_rotation(cam_h_rd)
    _, _, _, cam_h, aspect_h, fov_h = TR.camera(cam_h_rd)
    with np.errstate(all="ignore"):
        e = [X[..., k] - cam_h[k] for k in range(3)]
        Dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).astype(F32)
        v = [(rinv[k, 0] * e[0] + rinv[k, 1] * e[1]) + rinv[k, 2] * e[2] for k in range(3)]
        qx, qy = v[0] / -v[2], v[1] / -v[2]
        fx = ((qx / (aspect_h * fov_h) + F32(1)) / F32(2)) * F32(width) - F32(0.5)
        fy = ((F32(1) - qy / fov_h) / F32(2)) * F32(height) - F32(0.5)
    return fx.astype(F32), fy.astype(F32), Dist, v[2] < 0


# ---- srt_temporal_kernel<2, ...> ------------------------------------------------------------------------------------------
def reproject(cur, hist, cam_rd, normal_threshold=0.9, depth_threshold=0.05, ids=None, table=None, tri_ids=None, rows=None, h_rows=None):
    """temporal_ref.reproject with a table (srt_temporal_kernel<1, ...>) and the DEFORMED state: tri_ids (h, w) uint32 the
    frame's triangle indices, rows / h_rows (n, 3, 3) the world-vertex tables of the frame and of the history,
    table['first_row'] each shape's first row. A DEFORMED pixel is a moved one whose map is deform_map of its triangle."""
    height, width = cur["Z"].shape
    out = dict(h=np.zeros((height, width), F32), c=np.zeros((height, width, 3), F32), m1=np.zeros((height, width), F32),
               m2=np.zeros((height, width), F32), taps=np.zeros((height, width), np.int32), borderline=np.zeros((height, width), bool))
    n_shapes = len(table["state"])
    ids = np.asarray(ids, np.uint32)
    has_shape = ids < n_shapes
    sid = np.where(has_shape, ids, 0).astype(np.int64)
    state = np.where(has_shape, table["state"][sid] if n_shapes else 0, -1)
    out["state"] = state
    if not hist["valid"] or TR.invert_rotation(hist["camera"]) is None:
        return out
    same = TR.same_camera(cam_rd, hist["camera"])
    active = (cur["cov"] > 0) & np.all(np.isfinite(cur["c"]), axis=-1)
    N = cur["N"]
    rigid = state == MOVED
    deformed = state == DEFORMED
    moved = rigid | deformed
    B = table["B"][sid]
    with np.errstate(all="ignore"):
        t = [(B[..., k, 0] * N[..., 0] + B[..., k, 1] * N[..., 1]) + B[..., k, 2] * N[..., 2] for k in range(3)]
        ln = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]).astype(F32)
        len_ok = (ln > 0) & np.isfinite(ln)
        Nr = np.stack([t[k] / ln for k in range(3)], -1).astype(F32)  # normalise(B_s N_p)
    # the deformed pixels' triangles, now and in the history frame
    count = np.diff(np.append(table["first_row"], len(rows)))  # (rows of non-models: 0)
    tri = np.asarray(tri_ids, np.uint32).astype(np.int64)
    tri_ok = deformed & (tri < count[sid])
    row = np.where(tri_ok, table["first_row"][sid] + tri, 0)
    if len(rows):
        X = first_hit(cur["Z"], cam_rd, width, height)
        Xh, Nd, d_ok = deform_map(rows[row], h_rows[row], X, N)
    else:
        Xh, Nd, d_ok = np.zeros((height, width, 3), F32), N, np.zeros((height, width), bool)
    N = np.where(rigid[..., None], Nr, np.where(deformed[..., None], Nd, N)).astype(F32)
    active &= has_shape & (state != NO_HISTORY) & (~rigid | len_ok) & (~deformed | (tri_ok & d_ok))
    projected = moved if same else np.ones((height, width), bool)
    ys, xs = np.mgrid[0:height, 0:width]
    fx = fy = np.zeros((height, width), F32)
    Dist, front = cur["Z"], np.zeros((height, width), bool)
    if not same:
        fx, fy, Dist, front = TR.project(cur["Z"], cam_rd, hist["camera"], width, height)
    if rigid.any():
        pm = TR.project(cur["Z"], cam_rd, hist["camera"], width, height, A=table["A"][sid])
        fx, fy, Dist, front = (np.where(rigid, a, b) for a, b in zip(pm, (fx, fy, Dist, front)))
    if deformed.any():
        pm = project_point(Xh, hist["camera"], width, height)
        fx, fy, Dist, front = (np.where(deformed, a, b) for a, b in zip(pm, (fx, fy, Dist, front)))
    with np.errstate(all="ignore"):
        inside = front & (fx > F32(-1)) & (fx < F32(width)) & (fy > F32(-1)) & (fy < F32(height))
    active &= inside | ~projected
    fxs, fys = np.where(inside & projected, fx, F32(0)).astype(F32), np.where(inside & projected, fy, F32(0)).astype(F32)
    flx, fly = np.floor(fxs), np.floor(fys)
    ax, ay = (fxs - flx).astype(F32), (fys - fly).astype(F32)
    x0 = np.where(projected, flx.astype(np.int64), xs)
    y0 = np.where(projected, fly.astype(np.int64), ys)
    Dist = np.where(projected, Dist, cur["Z"]).astype(F32)
    for f in (fxs, fys):
        out["borderline"] |= active & projected & (np.abs(f - np.round(f)) < 1e-4)
    taps = []
    for k in range(4):
        wx = ax if k & 1 else F32(1) - ax
        wy = ay if k >> 1 else F32(1) - ay
        wgt = np.where(projected, (wx * wy).astype(F32), F32(1) if k == 0 else F32(0)).astype(F32)
        taps.append((x0 + (k & 1), y0 + (k >> 1), wgt, projected | (k == 0)))
    hc, hcount, hm1, hm2, hg = hist["colour"], hist["count"], hist["m1"], hist["m2"], hist["guide"]
    nt, dt = F32(normal_threshold), F32(depth_threshold)
    sw = np.zeros((height, width), F32)
    sc = np.zeros((height, width, 3), F32)
    sh, s1, s2 = (np.zeros((height, width), F32) for _ in range(3))
    for qx, qy, w, used in taps:
        ok = active & used & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
        jx, jy = np.clip(qx, 0, width - 1), np.clip(qy, 0, height - 1)
        g0, g1 = hg[jy, jx, 0], hg[jy, jx, 1]
        c = hc[jy, jx]
        ok &= (g1[..., 3] > 0) & np.all(np.isfinite(c), axis=-1)
        hs = np.asarray(hist["ids"], np.uint32)[jy, jx]
        hs_state = np.where(hs < n_shapes, table["state"][np.where(hs < n_shapes, hs, 0).astype(np.int64)], STATIC)
        ok &= np.where(moved, hs == ids, hs_state == STATIC)
        with np.errstate(all="ignore"):
            dt_ = (N[..., 0] * g0[..., 0] + N[..., 1] * g0[..., 1]) + N[..., 2] * g0[..., 2]
            dz = np.abs(g0[..., 3] - Dist)
            lim = dt * Dist
            out["borderline"] |= ok & (np.abs(dt_ - nt) <= F32(1e-5) * max(abs(nt), F32(1e-5)))
            out["borderline"] |= ok & (np.abs(dz - lim) <= F32(1e-5) * np.abs(lim))
        ok &= (dt_ >= nt) & (dz <= lim)
        wk = np.where(ok, w, F32(0)).astype(F32)
        with np.errstate(all="ignore"):
            sw = np.where(ok, sw + wk, sw)
            sc = np.where(ok[..., None], sc + wk[..., None] * c, sc)
            sh = np.where(ok, sh + wk * hcount[jy, jx], sh)
            s1 = np.where(ok, s1 + wk * hm1[jy, jx], s1)
            s2 = np.where(ok, s2 + wk * hm2[jy, jx], s2)
        out["taps"] += ok
    out["borderline"] |= (out["taps"] > 0) & (np.abs(sw - F32(0.01)) <= F32(1e-7))
    has = sw >= F32(0.01)
    with np.errstate(all="ignore"):
        one = np.where(has, sw, F32(1))
        out["h"] = np.where(has, sh / one, F32(0)).astype(F32)
        out["c"] = np.where(has[..., None], sc / one[..., None], F32(0)).astype(F32)
        out["m1"] = np.where(has, s1 / one, F32(0)).astype(F32)
        out["m2"] = np.where(has, s2 / one, F32(0)).astype(F32)
    return out


def temporal_setup(canvas, inputs, F, hist, cam_rd, history_limit=32, normal_threshold=0.9, depth_threshold=0.05, ids=None, table=None,
                   tri_ids=None, rows=None, h_rows=None):
    """temporal_ref.temporal_setup with the host's rule for the third kernel: the deform kernel when there is a history and
    a shape of the table is DEFORMED, else what the library launches with object motion alone."""
    if not (hist["valid"] and np.any(table["state"] == DEFORMED)):
        return TR.temporal_setup(canvas, inputs, F, hist, cam_rd, history_limit, normal_threshold, depth_threshold, ids=ids, table=table)
    cur = TR.frame(canvas, inputs, F)
    rep = reproject(cur, hist, cam_rd, normal_threshold, depth_threshold, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows)
    out = TR.integrate(cur, rep, history_limit)
    out["rep"], out["cur"] = rep, cur
    return out


# ---- the deformations the tests run --------------------------------------------------------------------------------------
def copy_tris(tris):
    return np.frombuffer(bytearray(tris.tobytes()), tris.dtype)


def wave(tris, start, count, k, amplitude=0.02, freq=3.0):
    """frame k of a smooth wave over the vertices of tris[start:start + count] (model space): each vertex moves along y and
    x by amplitude * sin(freq * position + phase(k)); k = 0 is the mesh as given. Normals are left as they are."""
    out = copy_tris(tris)
    if k == 0:
        return out
    p = np.asarray(tris["v"]["pos"][start:start + count], np.float64)[..., :3]
    q = p.copy()
    q[..., 1] += amplitude * np.sin(freq * p[..., 0] + 0.7 * k) * np.cos(freq * p[..., 2])
    q[..., 0] += 0.5 * amplitude * np.sin(freq * p[..., 1] + 0.4 * k)
    out["v"]["pos"][start:start + count, :, :3] = q.astype(F32)
    return out


def pull_vertex(tris, tri, vertex, k, step=(0.0, 0.03, 0.02)):
    """frame k: every vertex of tris that shares the position of vertex `vertex` of triangle `tri` moves by k * step"""
    out = copy_tris(tris)
    pos = np.asarray(tris["v"]["pos"], F32)[..., :3]
    same = np.all(pos == pos[tri, vertex], axis=-1)
    moved = pos.astype(np.float64)
    moved[same] += np.asarray(step, np.float64) * k
    out["v"]["pos"][..., :3] = moved.astype(F32)
    return out


def nearest_triangles(rows, org, dirs):
    """float64 Moeller-Trumbore of rays (org (3,), dirs (n, 3)) against world triangles rows (m, 3, 3): the index of the
    nearest hit per ray (-1: none). For the CPU tests' triangle indices; the device's come from the tracer's own test."""
    p0, e1, e2 = (np.float64(rows[:, 0]), np.float64(rows[:, 1]) - np.float64(rows[:, 0]), np.float64(rows[:, 2]) - np.float64(rows[:, 0]))
    d = np.float64(dirs)[:, None, :]
    with np.errstate(all="ignore"):
        pv = np.cross(d, e2[None])
        det = np.sum(e1[None] * pv, -1)
        tv = np.float64(org)[None, None, :] - p0[None]
        u = np.sum(tv * pv, -1) / det
        qv = np.cross(tv, e1[None])
        v = np.sum(d * qv, -1) / det
        t = np.sum(e2[None] * qv, -1) / det
        ok = (np.abs(det) > 1e-14) & (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (t > 1e-6)
    t = np.where(ok, t, np.inf)
    best = np.argmin(t, 1)
    return np.where(np.isfinite(t[np.arange(len(best)), best]), best, -1)


# (id, scene of gpu_harness.guide_scene / scene, acceleration, device upkeep, camera path, deformation, moves of motion_ref)
# deformation: ("pull", triangle, vertex) or ("wave", first triangle, count, amplitude)
CASES = [
    ("quad-pulled", "boxes", 0, False, None, ("pull", 0, 0), []),
    ("mesh-wave", "meshes", 0, False, None, ("wave", 12, 968, 0.02), []),
    ("wave-and-transform", "meshes", 1, False, None, ("wave", 12, 968, 0.02), [(1, "translate", (0.021, 0.009, -0.013))]),
    ("wave-camera", "meshes", 1, False, "move", ("wave", 12, 968, 0.02), []),
    ("wave-refit-scan", "meshes", 0, True, None, ("wave", 12, 968, 0.02), []),
    ("wave-refit-bvh", "meshes", 1, True, None, ("wave", 12, 968, 0.02), []),
    ("wave-beside-sphere", "mixed", 1, False, None, ("wave", 12, 200, 0.02), [(1, "translate", (0.019, 0.008, 0.011))]),
]
FRAMES, SIZE = 4, (37, 29)


def case_scene(name):
    from gpu_harness import guide_scene, scene
    return guide_scene(name)[:3] if name == "boxes" else scene(name)


def case_camera(name, k, kind):
    from gpu_harness import cam_at, guide_scene
    return guide_scene(name)[3] if name == "boxes" else cam_at(k, kind)


def case_frame(case, shapes, tris, k):
    """frame k of a case -> (shapes, triangles)"""
    deform, steps = case[5], case[6]
    now = pull_vertex(tris, deform[1], deform[2], k) if deform[0] == "pull" else wave(tris, deform[1], deform[2], k, deform[3])
    return M.move_shapes(shapes, tris, steps, k), now
