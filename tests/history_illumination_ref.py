"""The temporal set-up with the history reprojected as illumination (include/srt_abi.h srt_set_denoise_history_illumination;
srt_temporal_kernel of simple-raytracer_amd/csrc/temporal.hip with ILLUM true) in numpy: the tap loop of vertex_motion_ref.reproject --
the superset of the three kernels; without a table it is temporal_ref.reproject's -- with the rule

    D = max(A, SRT_DEMOD_EPS) per channel (fmaxf: a NaN channel gives eps), L = lum(D)
    a counted tap h of a pixel p that projects, cov_p == 1 and cov_h == 1:  r = D_p / D_h per channel, rl = L_p / L_h
    every other tap (a partly covered pixel or tap, the identity tap):      r = (1, 1, 1), rl = 1
    colour += w (c_h r),  m1 += w (m1_h rl),  m2 += w ((m2_h rl) rl)

Everything float32 in the kernel's order, unfused. The rule adds no test that could fall either way, so `borderline` and
`taps` are the colour path's. integrate is temporal_ref's, unchanged. rescale=False is the colour path (the anchor of
tests/test_history_illumination_reference.py); 'scaled' (h, w) counts the taps that were rescaled.
"""
import numpy as np

import demod_ref as DM
import denoise_ref as D
import temporal_ref as TR
import vertex_motion_ref as VM
from temporal_ref import MOVED, NO_HISTORY, STATIC
from vertex_motion_ref import DEFORMED

F32 = np.float32
EPS = DM.EPS  # SRT_DEMOD_EPS


def ratios(Ap, cov_p, Ah, cov_h):
    """r (..., 3), rl (...) float32 of a tap: D_p / D_h and lum(D_p) / lum(D_h) where both coverages are exactly 1, else 1;
    and the mask of the rescaled taps"""
    Dp, Dh = np.fmax(np.asarray(Ap, F32), EPS).astype(F32), np.fmax(np.asarray(Ah, F32), EPS).astype(F32)
    both = (np.asarray(cov_p, F32) == F32(1)) & (np.asarray(cov_h, F32) == F32(1))
    with np.errstate(all="ignore"):
        r = np.where(both[..., None], Dp / Dh, F32(1)).astype(F32)
        rl = np.where(both, D.lum(Dp) / D.lum(Dh), F32(1)).astype(F32)
    return r, rl, both


def reproject(cur, hist, cam_rd, normal_threshold=0.9, depth_threshold=0.05, ids=None, table=None, tri_ids=None, rows=None, h_rows=None,
              rescale=True):
    """-> temporal_ref.reproject's dict (h, c, m1, m2, taps, borderline; with a table also state) and 'scaled'. table None:
    srt_temporal_kernel<0, true, ...>; a table: srt_temporal_kernel<1, true, ...>; a table with DEFORMED rows and tri_ids, rows,
    h_rows: srt_temporal_kernel<2, true, ...> (arguments as vertex_motion_ref.reproject)."""
    height, width = cur["Z"].shape
    out = dict(h=np.zeros((height, width), F32), c=np.zeros((height, width, 3), F32), m1=np.zeros((height, width), F32),
               m2=np.zeros((height, width), F32), taps=np.zeros((height, width), np.int32), borderline=np.zeros((height, width), bool),
               scaled=np.zeros((height, width), np.int32))
    motion = table is not None
    if motion:
        n_shapes = len(table["state"])
        ids = np.asarray(ids, np.uint32)
        has_shape = ids < n_shapes
        sid = np.where(has_shape, ids, 0).astype(np.int64)
        state = np.where(has_shape, table["state"][sid] if n_shapes else 0, -1)
        out["state"] = state
    if not hist["valid"]:
        return out
    same = TR.same_camera(cam_rd, hist["camera"])
    if (motion or not same) and TR.invert_rotation(hist["camera"]) is None:
        return out
    active = (cur["cov"] > 0) & np.all(np.isfinite(cur["c"]), axis=-1)
    N = cur["N"]
    rigid = deformed = moved = np.zeros((height, width), bool)
    Xh = None
    if motion:
        rigid = state == MOVED
        deformed = (state == DEFORMED) if rows is not None else np.zeros((height, width), bool)
        moved = rigid | deformed
        B = table["B"][sid]
        with np.errstate(all="ignore"):
            t = [(B[..., k, 0] * N[..., 0] + B[..., k, 1] * N[..., 1]) + B[..., k, 2] * N[..., 2] for k in range(3)]
            ln = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]).astype(F32)
            len_ok = (ln > 0) & np.isfinite(ln)
            Nr = np.stack([t[k] / ln for k in range(3)], -1).astype(F32)  # normalise(B_s N_p)
        tri_ok = d_ok = np.zeros((height, width), bool)
        Nd = N
        if rows is not None and len(rows):
            count = np.diff(np.append(table["first_row"], len(rows)))
            tri = np.asarray(tri_ids, np.uint32).astype(np.int64)
            tri_ok = deformed & (tri < count[sid])
            row = np.where(tri_ok, table["first_row"][sid] + tri, 0)
            Xh, Nd, d_ok = VM.deform_map(rows[row], h_rows[row], VM.first_hit(cur["Z"], cam_rd, width, height), N)
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
        pm = VM.project_point(Xh, hist["camera"], width, height)
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
        if motion:  # a moved shape's tap must show that shape; a static one's must not show a shape that has left
            hs = np.asarray(hist["ids"], np.uint32)[jy, jx]
            hs_state = np.where(hs < n_shapes, table["state"][np.where(hs < n_shapes, hs, 0).astype(np.int64)], STATIC)
            ok &= np.where(moved, hs == ids, hs_state == STATIC)
        with np.errstate(all="ignore"):
            dot = (N[..., 0] * g0[..., 0] + N[..., 1] * g0[..., 1]) + N[..., 2] * g0[..., 2]
            dz = np.abs(g0[..., 3] - Dist)
            lim = dt * Dist
            out["borderline"] |= ok & (np.abs(dot - nt) <= F32(1e-5) * max(abs(nt), F32(1e-5)))
            out["borderline"] |= ok & (np.abs(dz - lim) <= F32(1e-5) * np.abs(lim))
        ok &= (dot >= nt) & (dz <= lim)
        # ---- the rule: the tap's colour and moments from its own albedo to the pixel's (never the identity tap) ----
        r, rl, both = ratios(cur["A"], cur["cov"], g1[..., :3], g1[..., 3])
        scale = both & projected & bool(rescale)
        r = np.where(scale[..., None], r, F32(1)).astype(F32)
        rl = np.where(scale, rl, F32(1)).astype(F32)
        wk = np.where(ok, w, F32(0)).astype(F32)
        with np.errstate(all="ignore"):
            sw = np.where(ok, sw + wk, sw)
            sc = np.where(ok[..., None], sc + wk[..., None] * (c * r), sc)
            sh = np.where(ok, sh + wk * hcount[jy, jx], sh)
            s1 = np.where(ok, s1 + wk * (hm1[jy, jx] * rl), s1)
            s2 = np.where(ok, s2 + wk * ((hm2[jy, jx] * rl) * rl), s2)
        out["taps"] += ok
        out["scaled"] += ok & scale
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
                   tri_ids=None, rows=None, h_rows=None, rescale=True):
    """The whole set-up with the host's rule for the kernel (vertex_motion_ref.temporal_setup's): the deform variant when
    there is a history and a shape of the table is DEFORMED, the motion variant when one is not STATIC, else the plain one."""
    cur = TR.frame(canvas, inputs, F)
    if not (table is not None and hist["valid"] and np.any(table["state"] != STATIC)):
        ids = table = None
    if table is None or not np.any(table["state"] == DEFORMED):
        tri_ids = rows = h_rows = None
    rep = reproject(cur, hist, cam_rd, normal_threshold, depth_threshold, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows,
                    rescale=rescale)
    out = TR.integrate(cur, rep, history_limit)
    out["rep"], out["cur"] = rep, cur
    return out
