"""The host side of the temporal stage's object motion (simple-raytracer_amd/csrc/temporal.hip, include/srt_abi.h
srt_set_denoise_object_motion) in numpy, and the moves the tests run.

table_row() is the per-shape table's float64 formulas; scene_table() the comparison that keeps or drops the history. The
moved set-up kernel itself is temporal_ref.reproject with ids and a table.
"""
import numpy as np

import temporal_ref as TR
from temporal_ref import MOVED, NO_HISTORY, STATIC  # noqa: F401 (the table's states, for the tests)

F32 = np.float32
NO_SHAPE = 0xFFFFFFFF
SPHERE, PLANE, MODEL = 0, 1, 2


# ---- the host's table ---------------------------------------------------------------------------------------------------
def _model_parts(shape):
    m = np.asarray(shape["transform"], np.float64)  # (4, 4): columns
    return m[:3, :3].T.copy(), m[3, :3].copy()


def table_row(hist, cur):
    """One shape's record in the history scene and now -> (state, A (3, 4) float64: current world -> history world,
    B (3, 3) float64: current normal -> history normal). The formulas of include/srt_abi.h, in float64."""
    eye = (np.hstack([np.eye(3), np.zeros((3, 1))]), np.eye(3))
    if hist.tobytes() == cur.tobytes():
        return (STATIC,) + eye
    kind = int(cur["type"])
    with np.errstate(all="ignore"):
        if kind == SPHERE:
            rh, rc = float(hist["sphere_radius"]), float(cur["sphere_radius"])
            if not (rh > 0 and rc > 0 and np.isfinite(rh) and np.isfinite(rc)):
                return (NO_HISTORY,) + eye
            s = rh / rc
            ph, pc = np.asarray(hist["sphere_position"], np.float64)[:3], np.asarray(cur["sphere_position"], np.float64)[:3]
            lin, tr, nrm = s * np.eye(3), ph - s * pc, (rc / rh) * np.eye(3)
        elif kind == PLANE:
            u, v = np.asarray(hist["plane_normal"], np.float64)[:3], np.asarray(cur["plane_normal"], np.float64)[:3]
            lu, lv = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            if not (lu > 0 and lv > 0 and np.isfinite(lu) and np.isfinite(lv)):
                return (NO_HISTORY,) + eye
            u, v = u / lu, v / lv
            k = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
            c = u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
            if not c > -1.0 + 1e-12:
                return (NO_HISTORY,) + eye
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            K2 = np.array([[sum(K[r][j] * K[j][q] for j in range(3)) for q in range(3)] for r in range(3)])
            Rm = np.eye(3) + K + K2 / (1.0 + c)  # history -> current
            ph, pc = np.asarray(hist["plane_position"], np.float64)[:3], np.asarray(cur["plane_position"], np.float64)[:3]
            lin = Rm.T.copy()
            tr = np.array([ph[r] - (lin[r][0] * pc[0] + lin[r][1] * pc[1] + lin[r][2] * pc[2]) for r in range(3)])
            nrm = lin
        else:
            (Lh, th), (Lc, tc) = _model_parts(hist), _model_parts(cur)
            if not (np.all(np.isfinite(th)) and np.all(np.isfinite(tc))):
                return (NO_HISTORY,) + eye
            Lci, Lhi = TR.inv3(Lc), TR.inv3(Lh)
            if Lci is None or Lhi is None:
                return (NO_HISTORY,) + eye
            lin = np.array([[(Lh[r][0] * Lci[0][q] + Lh[r][1] * Lci[1][q]) + Lh[r][2] * Lci[2][q] for q in range(3)] for r in range(3)])
            fwd = np.array([[(Lc[r][0] * Lhi[0][q] + Lc[r][1] * Lhi[1][q]) + Lc[r][2] * Lhi[2][q] for q in range(3)] for r in range(3)])
            tr = np.array([th[r] - ((lin[r][0] * tc[0] + lin[r][1] * tc[1]) + lin[r][2] * tc[2]) for r in range(3)])
            nrm = fwd.T.copy()
        A = np.hstack([lin, tr[:, None]])
        if not (np.all(np.isfinite(A.astype(F32))) and np.all(np.isfinite(nrm.astype(F32)))):
            return (NO_HISTORY,) + eye
    return MOVED, A, nrm


def scene_table(hist, cur):
    """hist, cur: (shapes, triangles, materials, scene_data) records. None = the history is dropped, else dict state (n,),
    A (n, 3, 4), B (n, 3, 3) rounded to float32."""
    (hs, ht, hm, hd), (cs, ct, cm, cd) = hist, cur
    if len(hs) != len(cs) or ht.tobytes() != ct.tobytes() or hm.tobytes() != cm.tobytes() or np.asarray(hd).tobytes() != np.asarray(cd).tobytes():
        return None
    for a, b in zip(hs, cs):
        if a["type"] != b["type"] or a["material"] != b["material"]:
            return None
        if int(a["type"]) == MODEL:
            for f in ("triangle_index", "num_triangles"):  # (the bounds are the world box: they follow the transform)
                if a[f] != b[f]:
                    return None
    rows = [table_row(a, b) for a, b in zip(hs, cs)]
    return dict(state=np.array([r[0] for r in rows], np.int64), A=np.array([r[1] for r in rows], np.float64).astype(F32).reshape(-1, 3, 4),
                B=np.array([r[2] for r in rows], np.float64).astype(F32).reshape(-1, 3, 3))


def static_table(n):
    return dict(state=np.zeros(n, np.int64), A=np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32), (n, 1, 1)),
                B=np.tile(np.eye(3, dtype=F32), (n, 1, 1)))


# ---- the moves tests/test_gpu_denoise_motion.py runs and tests/test_motion_reference.py checks the flagged share of ------
def rot_axis(axis, angle):
    """4x4 (records' column layout m[col][row]) rotation about a unit axis through the origin, float64"""
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                  [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                  [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])
    m = np.eye(4)
    m[:3, :3] = r.T
    return m


def _set_transform(shape, tris, m64):
    """a model record with another transform and the bounds the front-end derives from it"""
    from simple_raytracer_amd import records as R
    return R.model(int(shape["material"]), tris, int(shape["triangle_index"]), int(shape["num_triangles"]), np.asarray(m64, np.float64).astype(F32))


def _about(m64, centre, local):
    """local (4x4, column layout) applied about `centre`, after m64: T(c) local T(-c) m, as column-layout products"""
    t0, t1 = np.eye(4), np.eye(4)
    t0[3, :3], t1[3, :3] = -np.asarray(centre, np.float64), np.asarray(centre, np.float64)
    return m64 @ t0 @ local @ t1  # row-vector convention of the column layout: x' = x m


def move_shapes(base, tris, steps, k):
    """frame k of a move: `steps` = [(shape index, kind, amount per frame)]; kinds: translate (vector), scale (factor per
    frame about the sphere's centre / the model's origin), shift (plane, along its normal), tilt (plane, angle about x),
    rotate (model, angle about y through its origin)"""
    shapes = np.frombuffer(bytearray(base.tobytes()), base.dtype)  # (a copy of the bytes: .copy() drops the padding)
    for idx, kind, amount in steps:
        s = shapes[idx]
        typ = int(s["type"])
        if kind == "translate":
            d = np.asarray(amount, np.float64) * k
            if typ == SPHERE:
                s["sphere_position"][:3] = (np.asarray(base[idx]["sphere_position"][:3], np.float64) + d).astype(F32)
            elif typ == PLANE:
                s["plane_position"][:3] = (np.asarray(base[idx]["plane_position"][:3], np.float64) + d).astype(F32)
            else:
                m = np.asarray(base[idx]["transform"], np.float64).copy()
                m[3, :3] += d
                shapes[idx] = _set_transform(base[idx], tris, m)
        elif kind == "scale":
            f = float(amount) ** k
            if typ == SPHERE:
                s["sphere_radius"] = F32(float(base[idx]["sphere_radius"]) * f)
            else:
                m = np.asarray(base[idx]["transform"], np.float64)
                sc = np.diag([f, f * (1 + 0.3 * (f - 1)), f, 1.0])  # a little non-uniform
                shapes[idx] = _set_transform(base[idx], tris, _about(m, m[3, :3], sc))
        elif kind == "shift":
            n = np.asarray(base[idx]["plane_normal"][:3], np.float64)
            s["plane_position"][:3] = (np.asarray(base[idx]["plane_position"][:3], np.float64) + n / np.linalg.norm(n) * amount * k).astype(F32)
        elif kind == "tilt":
            r = rot_axis((1, 0, 0), amount * k)[:3, :3].T
            s["plane_normal"][:3] = (r @ np.asarray(base[idx]["plane_normal"][:3], np.float64)).astype(F32)
        elif kind == "rotate":
            m = np.asarray(base[idx]["transform"], np.float64)
            shapes[idx] = _set_transform(base[idx], tris, _about(m, m[3, :3], rot_axis((0, 1, 0), amount * k)))
        else:
            raise ValueError(kind)
    return shapes


# (id, scene, acceleration, camera path (None: still), steps). Shape indices: simple_raytracer_amd/scenes.py
MOVES = [
    ("sphere-translate", "spheres", 0, None, [(4, "translate", (0.031, 0.012, 0.02))]),
    ("sphere-scale-cam", "spheres", 0, "move", [(3, "scale", 1.02)]),
    # (with a still camera a floor or a wall shifted along its normal keeps one tap coordinate on whole pixels: all borderline)
    ("plane-shift", "spheres", 0, None, [(2, "shift", 0.013)]),
    ("plane-tilt-cam", "spheres", 0, "yaw", [(0, "tilt", 0.004)]),
    ("model-translate", "meshes", 0, None, [(1, "translate", (0.027, 0.011, -0.017))]),
    ("model-rotate-cam", "meshes", 1, "move", [(2, "rotate", 0.021)]),
    ("model-scale", "meshes", 1, None, [(1, "scale", 1.015)]),
    ("mixed", "mixed", 1, "move", [(1, "translate", (0.023, 0.0, 0.014)), (4, "rotate", 0.017), (7, "shift", 0.019)]),
]
FRAMES, SIZE = 4, (128, 72)  # frame 0 starts the history, frames 1 .. FRAMES - 1 move
