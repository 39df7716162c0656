"""GPU: the denoiser's spatial variance estimate (srt_set_denoise_spatial_variance) -- the filter with the estimate against
tests/spatial_variance_ref.py chained into the set-up, temporal and demodulation references, the estimate itself read back
through a one-pass filter that keeps each pixel to itself, pixels that do not qualify, off means unchanged, determinism, the
render paths, a device group, the error codes, srt_headless, and quality against 4096 spp with the switch-off filter as the
yardstick."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import spatial_variance_ref as SV
import temporal_ref as TR
from conftest import bits_equal
from gpu_harness import T, cam_at, guide_scene, make, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R
from test_gpu_denoise import check_filter, ground_truth

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (3, 2), (7, 7), (17, 19), (37, 21)]  # the window beyond every border; a tile seam with its halo in x, in y, in both
MIN_SAMPLES = (1, 3, 8, 1 << 20)
TP = dict(history_limit=32, normal_threshold=0.9, depth_threshold=0.05)
SELF_ONLY = dict(sigma_luminance=1e-20)  # a pass in which a tap with another luminance has weight 0


def handle(T, sky, name, w, h, temporal=None, **kw):
    shapes, tris, mats, cam = guide_scene(name)
    return make(T, sky, (shapes, tris, mats), w, h, spp=2, cam=cam, denoise={}, temporal=temporal, **kw)


def next_frame(t, cam, time):
    t.clear_canvas()
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam
    t.options["time"] = time
    return t.render(1).copy()


def setup_state(t, hist):
    """The set-up's output and the estimate's per-pixel inputs in numpy: spatial (hist None) or temporal. Where the temporal
    restatement flags a pixel as hanging on the last bit and the library decided it the other way, the library's staged
    values stand in for the restatement's (read back after the test's filters, by committing the frame)."""
    inp = t.read_denoise_inputs()
    canvas = t.read_canvas()
    if hist is None:
        c, V, N, Z, A, cov = D.setup(canvas, inp["normal_depth"], inp["albedo_hits"], inp["moments"], inp["T"], inp["P"], inp["T"], inp["T"])
        return dict(c=c, V=V, N=N, Z=Z, A=A, cov=cov, src=SV.sources_spatial(canvas, inp["moments"], inp["T"], inp["P"]))
    want = TR.temporal_setup(canvas, inp, inp["T"], hist, t.options, **TP)
    cur = want["cur"]
    return dict(c=want["c"], V=want["V"], N=cur["N"], Z=cur["Z"], A=cur["A"], cov=cur["cov"], src=SV.sources_staged(want["commit"]),
                commit=want["commit"], borderline=want["rep"]["borderline"])


def adopt_staged(st, got_h):
    """temporal: the staged set the library committed, where it differs from the restatement's (flagged pixels only)"""
    differs = np.zeros(st["cov"].shape, bool)
    for k in ("colour", "count", "m1", "m2"):
        a, b = got_h[k].view(np.uint32), st["commit"][k].view(np.uint32)
        differs |= (a != b).reshape(differs.shape + (-1,)).any(-1)
    assert not (differs & ~st["borderline"]).any()
    if differs.any():
        c, n, m1, m2 = got_h["colour"], got_h["count"], got_h["m1"], got_h["m2"]
        with np.errstate(all="ignore"):  # the set-up's variance from what it staged (counts below history_limit: n itself)
            v = m2 - m1 * m1
            v = np.where(v > 0, v, np.float32(0)) / n
            v = np.where(np.isfinite(v), v, np.float32(0)).astype(np.float32)
        st["c"] = np.where(differs[..., None], c, st["c"])
        st["V"] = np.where(differs, v, st["V"])
        st["src"] = tuple(np.where(differs, a, b) for a, b in zip((n, m1, m2), st["src"]))
    return int(differs.sum())


# ---- 1. against numpy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("name", ["spheres", "mesh_smooth"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_filter_with_estimate_matches_numpy(T, sky, w, h, name, temporal):
    t = handle(T, sky, name, w, h, temporal=TP if temporal else None)
    hist = None
    if temporal:  # one committed frame, then a moved camera: the counts differ per pixel
        t.options["camera_to_world"] = cam_at(0, "move")
        t.render(1)
        t.clear_canvas()
        hist = t.read_denoise_history()
        t.update_scene(*t.scene)
        t.options["camera_to_world"] = cam_at(3, "move")
        t.options["time"] = 2001
    t.render(1)
    st = setup_state(t, hist)
    runs = []
    for demod in (False, True):
        t.set_denoise_demodulation(demod)
        for K, sig in ((1, {}), (5, {}), (1, SELF_ONLY)):
            for ms in MIN_SAMPLES:
                t.set_denoise(iterations=K, **sig)
                t.set_denoise_spatial_variance(ms)  # (set_denoise with the denoiser on keeps the switch)
                t.resolve_denoised(1)
                t.synchronize()
                assert t.last_filter_spatial_variance() and t.last_filter_demodulated() == demod
                runs.append((demod, K, sig, ms, t.read_denoised(), t.read_argb().reshape(h, w, 4).copy()))
    if temporal:
        t.clear_canvas()
        adopt_staged(st, t.read_denoise_history())
    qualified = 0
    for demod, K, sig, ms, got, argb in runs:
        what = f"{w}x{h} {name} temporal={temporal} demod={demod} K={K} {sig} min_samples={ms}"
        steps, after = SV.filter_steps(st["c"], st["V"], st["N"], st["Z"], st["A"], st["cov"], *st["src"], ms, iterations=K, demod=demod, **sig)
        check_filter(got, argb, *steps[K], what)
        q = SV.qualifies(after[..., :3], st["cov"], st["src"][0], ms)
        qualified += int(q.sum())
        if sig:
            # the estimate itself: in this pass a pixel none of whose 24 taps shares its luminance is its own only tap, so
            # what comes out is {colour, variance} as they stood right after the estimate's launch
            lum = D.lum(np.where(np.isfinite(after[..., :3]), after[..., :3], 0))
            alone = np.ones((h, w), bool)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if (dx or dy):
                        ys, xs = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
                        inside = ((np.arange(h) + dy == ys)[:, None]) & ((np.arange(w) + dx == xs)[None, :])
                        alone &= ~inside | (np.abs(lum[ys][:, xs] - lum) > 1e-6)
            pin = q & alone
            V_after = after[..., 3]
            if demod:  # the last pass multiplied the albedo's luminance back
                V_after = V_after * D.lum(np.fmax(st["A"], np.float32(0.01))) ** 2
            np.testing.assert_allclose(got[..., 3][pin], V_after[pin], rtol=1e-3, atol=1e-9, err_msg=what)
            if q.sum() >= 20:
                assert pin.sum() >= 0.5 * q.sum(), what
    if w * h >= 49:
        assert qualified > 0
    t.close()


# ---- 2. pixels that do not qualify ----------------------------------------------------------------------------------------
def test_pixels_with_history_are_untouched(T, sky):
    w, h = 64, 40
    on, off = (handle(T, sky, "spheres", w, h, temporal=TP) for _ in range(2))
    for t in (on, off):
        t.set_denoise(iterations=1)
    on.set_denoise_spatial_variance(2 + 1)  # P + 1: the second frame's pixels with history have 4 samples
    for f in range(2):
        outs = [next_frame(t, guide_scene("spheres")[3], 50 + f) for t in (on, off)]
        a, b = on.read_denoised(), off.read_denoised()
        assert on.last_filter_spatial_variance() and not off.last_filter_spatial_variance()
        if f == 0:  # no history anywhere: every first hit qualifies
            assert not bits_equal(a[..., 3], b[..., 3])
    on.clear_canvas()
    hist = on.read_denoise_history()
    q = (hist["count"] < 3) & (hist["guide"][..., 1, 3] > 0)  # the pixels the second frame estimated
    near = np.zeros((h, w), bool)  # within one pass's reach of such a pixel
    for y, x in np.argwhere(q):
        near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
    # (a still camera keeps most histories; the feature ray's jitter moves first hits across silhouettes, which drops some)
    print(f"second frame: {q.mean() * 100:.1f}% of the pixels estimated, {(~near).mean() * 100:.1f}% out of their reach")
    assert q.any() and (hist["count"] == 4).any() and (~near).mean() > 0.25
    assert bits_equal(a[~near], b[~near])
    assert np.array_equal(outs[0].reshape(h, w, 4)[~near], outs[1].reshape(h, w, 4)[~near])
    for t in (on, off):
        t.close()


# ---- 3. off is off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temporal", [False, True])
def test_off_is_off(T, sky, temporal):
    w, h = 64, 40
    tp = TP if temporal else None
    never, zero, low, on = (handle(T, sky, "mesh_smooth", w, h, temporal=tp) for _ in range(4))
    zero.set_denoise_spatial_variance(8)
    zero.set_denoise_spatial_variance(0)
    low.set_denoise_spatial_variance(2)  # <= P = 2: without temporal no pixel has fewer samples
    on.set_denoise_spatial_variance(8)
    for f in range(3):
        outs = [next_frame(t, cam_at(f, "move"), 90 + f) for t in (never, zero, low, on)]
        assert np.array_equal(outs[0], outs[1]) and bits_equal(never.read_denoised(), zero.read_denoised()), f
        assert not zero.last_filter_spatial_variance() and low.last_filter_spatial_variance() and on.last_filter_spatial_variance()
        if not temporal:
            assert np.array_equal(outs[0], outs[2]) and bits_equal(never.read_denoised(), low.read_denoised()), f
        assert not bits_equal(never.read_denoised()[..., 3], on.read_denoised()[..., 3]), f
        # the canvas, the denoiser's inputs and (below) the history do not know about the switch
        assert bits_equal(never.read_canvas(), on.read_canvas()), f
        ia, ib = never.read_denoise_inputs(), on.read_denoise_inputs()
        for k in ("normal_depth", "albedo_hits", "moments"):
            assert bits_equal(ia[k], ib[k]), (f, k)
        if temporal:
            for t in (never, on):
                t.clear_canvas()
            ha, hb = never.read_denoise_history(), on.read_denoise_history()
            for k in ("colour", "count", "m1", "m2", "guide"):
                assert bits_equal(ha[k], hb[k]), (f, k)
    # K = 0: nothing is launched, the plain render's bytes, the set-up's variance
    plain = make(T, sky, guide_scene("mesh_smooth")[:3], w, h, spp=2, cam=cam_at(2, "move"), time=92)
    want = plain.render(1)
    for t in (never, on):
        t.set_denoise(iterations=0)
    on.set_denoise_spatial_variance(8)
    if temporal:  # (the frame was committed above: trace it again, without a history)
        for t in (never, on):
            t.reset_denoise_history()
            t.options["time"] = 92
            assert np.array_equal(t.render(1), want)
    else:
        for t in (never, on):
            t.resolve_denoised(1)
            t.synchronize()
            assert np.array_equal(t.read_argb().reshape(-1), want.reshape(-1))
    assert not on.last_filter_spatial_variance()
    assert bits_equal(never.read_denoised(), on.read_denoised())
    for t in (never, zero, low, on, plain):
        t.close()


# ---- 4. determinism and paths ---------------------------------------------------------------------------------------------
def test_two_filters_identical(T, sky):
    t = handle(T, sky, "mesh_smooth", 96, 64)
    t.set_denoise_spatial_variance(8)
    t.render(1)
    a, ha = t.read_argb().copy(), t.read_denoised()
    t.resolve_denoised(1)
    t.synchronize()
    assert np.array_equal(a, t.read_argb()) and bits_equal(ha, t.read_denoised())
    t.close()


def test_async_and_pipelined_equal_blocking(T, sky):
    w, h = 96, 64
    blk, asy, pip = (handle(T, sky, "spheres", w, h, temporal=TP) for _ in range(3))
    want, got_async, got_pipe = [], [], {}
    buf = np.zeros(w * h * 4, np.uint8)
    for i in range(4):
        for t in (blk, asy, pip):
            t.set_denoise_spatial_variance(8)
            t.clear_canvas()
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(i, "yaw")
            t.options["time"] = 70 + i
        want.append(blk.render(1).copy())
        o = np.zeros(w * h * 4, np.uint8)
        asy.render_async(1, o)
        asy.synchronize()
        got_async.append(o)
        n = pip.render_pipelined(1, buf)
        if n >= 0:
            got_pipe[n] = buf.copy()
    n = pip.pipeline_flush(buf)
    got_pipe[n] = buf.copy()
    for i in range(4):
        assert np.array_equal(want[i], got_async[i]), i
        assert np.array_equal(want[i], got_pipe[i]), i
    for t in (blk, asy, pip):
        assert t.last_filter_spatial_variance()
        t.close()


@pytest.mark.parametrize("temporal", [False, True])
def test_virtual_group_equals_single_handle(T, sky, temporal):
    w, h = 61, 29
    shapes, tris, mats, cam = guide_scene("mesh_smooth")
    ts = []
    for k in range(2):
        t = T.Tracer(w, h) if k == 0 else T.TracerGroup(w, h, n_devices=3, devices=[0, 0, 0], rows_per_block=5)
        t.set_skybox(sky)
        t.set_acceleration(1)
        t.options = R.render_data(w, h, 2, 10, camera_to_world=cam, time=777)
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        t.set_denoise()
        if temporal:
            t.set_denoise_temporal(**TP)
        t.set_denoise_spatial_variance(8)
        ts.append(t)
    for f in range(3):
        outs = []
        for t in ts:
            t.clear_canvas()
            t.update_scene(shapes, tris, mats)
            t.options["camera_to_world"] = cam_at(f, "move")
            t.options["time"] = 300 + f
            outs.append(t.render(1).copy())
        assert np.array_equal(outs[0], outs[1]), f
        assert bits_equal(ts[0].read_denoised(), ts[1].read_denoised()), f
        assert ts[0].last_filter_spatial_variance() and ts[1].last_filter_spatial_variance()
    for t in ts:
        t.close()


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def test_error_codes(T, sky):
    lib = T.load_library()
    t = make(T, sky, "spheres", 64, 48, spp=1)
    ran = C.c_int(7)
    assert lib.srt_set_denoise_spatial_variance(t._h, 8) == 3  # the denoiser is off
    assert lib.srt_set_denoise_spatial_variance(t._h, 0) == 0
    assert lib.srt_set_denoise_spatial_variance(None, 8) == 1 and lib.srt_last_filter_spatial_variance(t._h, None) == 1
    assert lib.srt_last_filter_spatial_variance(t._h, C.byref(ran)) == 0 and ran.value == 0
    t.set_denoise()
    assert lib.srt_set_denoise_spatial_variance(t._h, (1 << 20) + 1) == 1
    assert lib.srt_set_denoise_spatial_variance(t._h, 1 << 20) == 0
    t.render(1)
    assert t.last_filter_spatial_variance()
    t.set_denoise(False)  # turns the switch off with the denoiser
    t.set_denoise()
    t.render(1)
    assert not t.last_filter_spatial_variance()
    t.close()
    g = T.TracerGroup(64, 48, n_devices=2, devices=[0, 0], rows_per_block=8)
    assert lib.srt_group_set_denoise_spatial_variance(g._g, 8) == 3  # the group's denoiser is off
    assert lib.srt_group_set_denoise_spatial_variance(g._g, 0) == 0
    g.set_denoise()
    assert lib.srt_set_denoise_spatial_variance(g.member(0), 8) == 3  # a member of a group of more than one
    assert lib.srt_group_set_denoise_spatial_variance(g._g, (1 << 20) + 1) == 1
    assert lib.srt_group_set_denoise_spatial_variance(g._g, 8) == 0
    assert lib.srt_group_last_filter_spatial_variance(g._g, C.byref(ran)) == 0 and ran.value == 0
    assert lib.srt_group_set_denoise_spatial_variance(None, 8) == 1
    g.close()


def test_headless_spatial_variance_writes_ppm(tmp_path):
    from simple_raytracer_amd import build
    exe = build.build_headless()
    out = tmp_path / "v.ppm"
    subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", "2", "--denoise", "5",
                    "--spatial-variance", "8", "--out", str(out)], check=True, timeout=120)
    data = out.read_bytes()
    assert data.startswith(b"P6") and len(data) > 64 * 48 * 3
    assert subprocess.run([str(exe), "--scene", "spheres", "--spatial-variance", "8"], capture_output=True, timeout=120).returncode != 0


# ---- 6. quality -------------------------------------------------------------------------------------------------------------
# MSE_on / MSE_off against 4096 spp, tonemapped, min_samples = 8, as scripts/spatial_variance_probe.py measured them
# (profiles/r18_spatial_variance_quality.json). A ratio below 1 is held to the midpoint between it and 1; one that is not
# is only held below 1.05: the switch does no harm there, and nothing is claimed for it.
MEASURED = {"first_spheres": 0.6277, "first_meshes": 0.7037, "moving_spheres": 0.9830, "moving_spheres_no_history": 0.8652,
            "moving_meshes": 1.0069, "moving_meshes_no_history": 0.9673}


def bound(key):
    r = MEASURED[key]
    return (r + 1.0) / 2 if r < 1.0 else 1.05


_truth = {}


def first_frame_ratio(T, sky, name, accel):
    w, h = 160, 90
    if (name, accel) not in _truth:
        _truth[name, accel] = tone(ground_truth(T, sky, name, w, h, accel)[0])
    ref = _truth[name, accel]
    mse = []
    for ms in (0, 8):
        t = make(T, sky, name, w, h, spp=2, accel=accel, denoise={}, time=31)
        t.set_denoise_spatial_variance(ms)
        t.render(1)
        mse.append(float(np.mean((tone(t.read_denoised()[..., :3]) - ref) ** 2)))
        t.close()
    return mse[1] / mse[0], mse


def moving_camera_ratios(T, sky, name, accel):
    """the eighth frame of tests/test_gpu_denoise_temporal.py's moving-camera sequence: whole frame, pixels without history"""
    w, h, frames = 160, 90, 8
    g = make(T, sky, name, w, h, spp=4096, accel=accel, time=4242)
    g.options["camera_to_world"] = cam_at(frames - 1, "move")
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    off = make(T, sky, name, w, h, accel=accel, denoise={}, temporal={})
    on = make(T, sky, name, w, h, accel=accel, denoise={}, temporal={})
    on.set_denoise_spatial_variance(8)
    for k in range(frames):
        for t in (off, on):
            next_frame(t, cam_at(k, "move"), 900 + k)
    a, b = tone(off.read_denoised()[..., :3]), tone(on.read_denoised()[..., :3])
    on.clear_canvas()
    hist = on.read_denoise_history()
    dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)
    for t in (off, on):
        t.close()
    whole = float(np.mean((b - ref) ** 2)) / float(np.mean((a - ref) ** 2))
    part = float(np.mean((b[dis] - ref[dis]) ** 2)) / float(np.mean((a[dis] - ref[dis]) ** 2))
    return whole, part, float(dis.mean())


@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 1)])
def test_quality_first_frame(T, sky, name, accel):
    ratio, mse = first_frame_ratio(T, sky, name, accel)
    print(f"{name}: first 2-spp frame, MSE off {mse[0]:.4e}, on {mse[1]:.4e}, ratio {ratio:.4f}")
    assert ratio < bound(f"first_{name}")


@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 1)])
def test_quality_moving_camera(T, sky, name, accel):
    whole, part, share = moving_camera_ratios(T, sky, name, accel)
    print(f"{name}: eighth moving frame, ratio {whole:.4f} over the frame, {part:.4f} over the {share * 100:.1f}% of pixels without history")
    assert whole < bound(f"moving_{name}")
    assert part < bound(f"moving_{name}_no_history")
