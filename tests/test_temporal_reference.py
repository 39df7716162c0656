"""CPU: the numpy restatement of the denoiser's temporal reprojection (tests/temporal_ref.py) on analytic cases, and the
ctypes mirror of srt_temporal_params against include/srt_types.h."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import denoise_ref as D
import temporal_ref as TR
from simple_raytracer_amd import records as R
from simple_raytracer_amd.tracer import TemporalParams

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


def rd(w, h, cam):
    return R.render_data(w, h, 2, 10, camera_to_world=cam)


def frame_of(c, N, Z, cov=None, P=2, m2=None):
    """a current frame from its set-up values directly"""
    c = np.asarray(c, F32)
    h, w = Z.shape
    cov = np.ones((h, w), F32) if cov is None else np.asarray(cov, F32)
    m1 = D.lum(c)
    m2 = (m1 * m1 + F32(0.5)).astype(F32) if m2 is None else m2
    return dict(c=c, m1=m1, m2=m2, V=np.zeros((h, w), F32), N=np.asarray(N, F32), Z=np.asarray(Z, F32),
                A=np.full((h, w, 3), 0.5, F32), cov=cov, P=P)


def history_of(cur, colour, count, cam):
    h, w = cur["Z"].shape
    g = np.zeros((h, w, 2, 4), F32)
    g[..., 0, :3], g[..., 0, 3], g[..., 1, 3] = cur["N"], cur["Z"], 1.0
    return dict(valid=True, colour=np.asarray(colour, F32), count=np.full((h, w), count, F32), m1=D.lum(colour),
                m2=(D.lum(colour) ** 2).astype(F32), guide=g, camera=cam)


def plane_frame(w, h, L, cam_rd, P=2):
    """a plane z = -L facing the camera at the origin's height, seen from cam_rd: Z along each pixel's unit ray"""
    c0, c1, c2, cam, aspect, fov = TR.camera(cam_rd)
    ys, xs = np.mgrid[0:h, 0:w]
    sx = ((2 * (xs + 0.5) / w - 1) * aspect) * fov
    sy = (1 - 2 * (ys + 0.5) / h) * fov
    d = np.stack([sx, sy, -np.ones_like(sx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    Z = ((cam[2] + L) / -d[..., 2]).astype(F32)
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1
    c = np.random.RandomState(3).uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    return frame_of(c, N, Z, P=P)


def test_identity_camera_is_count_weighted_mean():
    w, h = 24, 16
    rng = np.random.RandomState(1)
    cam = rd(w, h, R.camera_matrix((0.0, 0.5, 5.0), 0.3, -0.1))
    N = np.zeros((h, w, 3), F32)
    N[..., 1] = 1
    cur = frame_of(rng.uniform(0, 3, (h, w, 3)), N, rng.uniform(1, 9, (h, w)), P=3)
    hist = history_of(cur, rng.uniform(0, 3, (h, w, 3)), 5.0, cam)
    rep = TR.reproject(cur, hist, cam)
    assert np.all(rep["taps"] == 1) and not rep["borderline"].any()
    assert np.array_equal(rep["c"], hist["colour"]) and np.all(rep["h"] == 5.0)
    out = TR.integrate(cur, rep, history_limit=4)  # the cap: h' = 4
    want = (3.0 * cur["c"].astype(np.float64) + 4.0 * hist["colour"]) / 7.0
    assert np.allclose(out["c"], want, rtol=1e-6)
    m1 = (3.0 * cur["m1"].astype(np.float64) + 4.0 * hist["m1"]) / 7.0
    m2 = (3.0 * cur["m2"].astype(np.float64) + 4.0 * hist["m2"]) / 7.0
    assert np.allclose(out["V"], np.maximum(0, m2 - m1 * m1) / 7.0, rtol=1e-4, atol=1e-6)
    assert np.all(out["commit"]["count"] == 4.0) and np.all(out["h"] == 4.0)


def test_translated_camera_taps_land_analytically():
    w, h, L = 64, 36, 4.0
    cam_h = rd(w, h, R.camera_matrix((0.0, 0.0, 0.0)))
    pix = 2.0 * (w / h) * L / w  # one pixel's width on the plane
    for k in (1, 3, -2):
        cam = rd(w, h, R.camera_matrix((k * pix, 0.0, 0.0)))
        cur = plane_frame(w, h, L, cam)
        fx, fy, Dist, front = TR.project(cur["Z"], cam, cam_h, w, h)
        xs = np.arange(w)[None, :] + k
        assert front.all()
        assert np.abs(fx - xs).max() < 2e-3 and np.abs(fy - np.arange(h)[:, None]).max() < 2e-3, k
        # the history sees the same plane: D equals the history camera's own distance along its ray
        hist_frame = plane_frame(w, h, L, cam_h)
        inside = (xs >= 0) & (xs < w)
        assert np.allclose(Dist[:, (xs[0] >= 0) & (xs[0] < w)], hist_frame["Z"][:, xs[0][inside[0]]], rtol=1e-5)
        hist = history_of(hist_frame, hist_frame["c"], 6.0, cam_h)
        rep = TR.reproject(cur, hist, cam)
        has = rep["h"] > 0
        assert np.array_equal(has, np.broadcast_to(inside, has.shape)), k
        # the colour moved with the plane: pixel x now holds the history's pixel x + k (within the bilinear residue)
        src = hist["colour"][:, xs[0][inside[0]]]
        assert np.allclose(rep["c"][:, inside[0]], src, rtol=2e-2, atol=2e-2)


def test_taps_behind_camera_and_outside_image_rejected():
    w, h, L = 32, 18, 4.0
    cam = rd(w, h, R.camera_matrix((0.0, 0.0, 0.0)))
    cur = plane_frame(w, h, L, cam)
    # the history camera stands beyond the plane, looking the same way: every point lies behind it
    behind = rd(w, h, R.camera_matrix((0.0, 0.0, -2 * L)))
    hist = history_of(cur, cur["c"], 4.0, behind)
    fx, fy, Dist, front = TR.project(cur["Z"], cam, behind, w, h)
    assert not front.any()
    assert np.all(TR.reproject(cur, hist, cam)["h"] == 0)
    # moved far sideways: every tap falls outside the history image
    far = rd(w, h, R.camera_matrix((1000.0, 0.0, 0.0)))
    hist = history_of(cur, cur["c"], 4.0, far)
    assert np.all(TR.reproject(cur, hist, cam)["h"] == 0)
    # a singular history camera: no history at all
    sing = rd(w, h, np.zeros((4, 4), F32))
    assert TR.invert_rotation(sing) is None
    assert np.all(TR.reproject(cur, history_of(cur, cur["c"], 4.0, sing), cam)["h"] == 0)


def test_rejection_on_normal_and_depth():
    w, h = 16, 8
    cam = rd(w, h, R.camera_matrix((0.0, 0.5, 5.0)))
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1
    cur = frame_of(np.ones((h, w, 3)), N, np.full((h, w), 2.0, F32))
    hist = history_of(cur, np.full((h, w, 3), 3.0, F32), 4.0, cam)
    hist["guide"][:, : w // 2, 0, :3] = [0, 1, 0]         # normals at 90 degrees: rejected
    hist["guide"][: h // 2, w // 2:, 0, 3] = 2.0 * 1.06   # 6 % farther: rejected at depth_threshold 0.05
    hist["guide"][h // 2:, w // 2:, 0, 3] = 2.0 * 1.04   # 4 %: kept
    rep = TR.reproject(cur, hist, cam)
    assert np.all(rep["h"][:, : w // 2] == 0) and np.all(rep["h"][: h // 2, w // 2:] == 0)
    assert np.all(rep["h"][h // 2:, w // 2:] == 4.0)


def test_no_history_is_the_spatial_setup():
    w, h = 20, 12
    rng = np.random.RandomState(7)
    T, P, F = 3, 7, 3
    canvas = rng.uniform(0, 5, (h, w, 4)).astype(F32)
    canvas[2, 3, 0] = np.inf
    nd = rng.uniform(-1, 1, (h, w, 4)).astype(F32)
    ah = rng.uniform(0, 1, (h, w, 4)).astype(F32)
    ah[..., 3] = rng.randint(0, 4, (h, w))
    moments = rng.uniform(0, 30, (h, w)).astype(F32)
    inputs = dict(normal_depth=nd, albedo_hits=ah, moments=moments, T=T, P=P)
    cam = rd(w, h, R.camera_matrix((0.0, 0.5, 5.0)))
    for hist in (dict(valid=False), dict(valid=True, camera=cam, **{k: v for k, v in history_of(
            TR.frame(canvas, inputs, F), canvas[..., :3], 5.0, cam).items() if k not in ("valid", "camera")})):
        out = TR.temporal_setup(canvas, inputs, F, hist, cam)
        c, V, N, Z, A, cov = D.setup(canvas, nd, ah, moments, T, P, F, T)
        none = out["h"] == 0
        if not hist["valid"]:
            assert none.all()
        else:
            hist["guide"][:, :, 1, 3] = np.where(cov > 0, 1.0, 0.0)
            assert none.any() and (~none).any()
        assert np.array_equal(out["c"][none].view(np.uint32), c[none].view(np.uint32))
        assert np.array_equal(out["V"][none].view(np.uint32), V[none].view(np.uint32))
        assert np.array_equal(out["commit"]["guide"][..., 0, 3], Z) and np.array_equal(out["commit"]["guide"][..., 1, 3], cov)
        assert np.all(out["commit"]["count"][none] == P)


def test_struct_layout_matches_header():
    text = (ROOT / "include/srt_types.h").read_text()
    assert int(re.search(r"sizeof\(srt_temporal_params\) == (\d+)", text).group(1)) == C.sizeof(TemporalParams) == 32
    offs = dict(re.findall(r"offsetof\(srt_temporal_params, (\w+)\) == (\d+)", text))
    assert len(offs) == 4
    for name, off in offs.items():
        assert getattr(TemporalParams, name).offset == int(off), name
    body = re.search(r"typedef struct srt_temporal_params \{(.*?)\} srt_temporal_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*\w+\s+(\w+)(?:\[\d+\])?;", body, re.M)
    assert fields == [n for n, _ in TemporalParams._fields_]


def test_defaults_from_the_library():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    d = tracer.temporal_defaults()
    assert d == dict(enable=1, history_limit=TR.DEFAULTS["history_limit"], normal_threshold=np.float32(TR.DEFAULTS["normal_threshold"]),
                     depth_threshold=np.float32(TR.DEFAULTS["depth_threshold"]), reserved=[0, 0, 0, 0])
