"""GPU: the denoiser's temporal reprojection (srt_set_denoise_temporal) -- off and no-history mean the spatial denoiser bit
for bit, a still camera against tests/temporal_ref.py bit for bit, a moving camera against it bit for bit on the pixels it does not flag, the
rules that drop the history, quality on a moving camera, the render paths, determinism, srt_headless and the error codes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import temporal_cases as TC
import temporal_ref as TR
from conftest import bits_equal
from gpu_harness import T, cam_at, make, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu


def next_frame(t, k, kind, time):
    """the front-end while moving: clear, update_scene (the same bytes), a new camera, one dispatch"""
    t.clear_canvas()
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam_at(k, kind)
    t.options["time"] = time
    return t.render(1).copy()


def frame_ref(t, hist, **tp):
    inp = t.read_denoise_inputs()
    return TR.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, **tp)


def check_commit(got, commit):
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(got[k], commit[k]), k


# ---- 1. off means unchanged ----------------------------------------------------------------------------------------------
def test_off_and_disabled_equal_spatial(T, sky):
    w, h = 96, 64
    spatial = make(T, sky, "mixed", w, h, denoise={})
    toggled = make(T, sky, "mixed", w, h, denoise={}, temporal={})
    toggled.set_denoise_temporal(False)
    on = make(T, sky, "mixed", w, h, denoise={}, temporal={})
    for k in range(3):
        outs = [next_frame(t, k, "move", 300 + k) for t in (spatial, toggled, on)]
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(spatial.read_denoised(), toggled.read_denoised()), k
        assert bits_equal(spatial.read_canvas(), on.read_canvas()), k  # the canvas is untouched by the temporal stage
        if k == 0:  # nothing to reproject yet
            assert np.array_equal(outs[0], outs[2]) and bits_equal(spatial.read_denoised(), on.read_denoised())
        else:
            assert not np.array_equal(outs[0], outs[2])
    for t in (spatial, toggled, on):
        t.close()


# ---- 2. no history means spatial ---------------------------------------------------------------------------------------
def test_no_history_equals_spatial(T, sky):
    w, h = 96, 64
    spatial = make(T, sky, "spheres", w, h, denoise={})
    temporal = make(T, sky, "spheres", w, h, denoise={}, temporal={})
    for k in range(4):
        if k == 2:
            temporal.clear_canvas()
            temporal.reset_denoise_history()
            assert not temporal.read_denoise_history()["valid"]
        a, b = (next_frame(t, k, "yaw", 500 + k) for t in (spatial, temporal))
        same = np.array_equal(a, b) and bits_equal(spatial.read_denoised(), temporal.read_denoised())
        assert same == (k in (0, 2)), k
    spatial.close()
    temporal.close()


# ---- 3. still camera, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit,spp", [(32, 2), (5, 2), (1, 3)])
def test_still_camera_bit_exact(T, sky, limit, spp):
    w, h = 80, 48
    tp = dict(history_limit=limit, normal_threshold=0.9, depth_threshold=0.05)
    t = make(T, sky, "mixed", w, h, spp=spp, denoise=dict(iterations=0), temporal=tp)
    hist = dict(valid=False)
    for f in range(5):
        dispatches = 2 if f == 3 else 1  # one frame of two dispatches (ticks = T = 2)
        for d in range(dispatches):
            t.options["time"] = 1000 + 17 * f + d
            argb = t.render(d + 1).copy()
        want = frame_ref(t, hist, **tp)
        got = t.read_denoised()
        assert bits_equal(got[..., :3], want["c"]), f
        assert bits_equal(got[..., 3], want["V"]), f
        assert np.array_equal(argb.reshape(h, w, 4), D.tonemap(want["c"])), f
        if f:
            assert (want["rep"]["taps"][want["cur"]["cov"] > 0] == 1).mean() > 0.9
            assert want["h"].max() == min(limit, hist["count"].max())
        t.clear_canvas()
        got_h = t.read_denoise_history()
        assert got_h["valid"]
        check_commit(got_h, want["commit"])
        assert got_h["camera"].tobytes() == t.options.tobytes()
        hist = got_h
    assert hist["count"].max() == min(limit, 6 * spp)  # 6 dispatches: the cap is reached where it is below that
    t.close()


def test_commit_without_a_filter_integrates_at_the_clear(T, sky):
    """trace alone, then clear: the clear integrates what the filter would have"""
    w, h = 64, 40
    a = make(T, sky, "mixed", w, h, denoise={}, temporal={})
    b = make(T, sky, "mixed", w, h, denoise={}, temporal={})
    for k in range(3):
        for t in (a, b):
            t.options["camera_to_world"] = cam_at(k, "move")
            t.options["time"] = 40 + k
        a.render(1)
        b.trace()
        for t in (a, b):
            t.clear_canvas()
        ha, hb = a.read_denoise_history(), b.read_denoise_history()
        check_commit(ha, hb)
    a.close()
    b.close()


# ---- 4. moving camera against numpy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel,kind", [("spheres", 0, "move"), ("spheres", 0, "yaw"), ("meshes", 0, "move"), ("meshes", 1, "pitch"),
                                             ("mixed", 0, "yaw"), ("mixed", 1, "move")])
def test_moving_camera_matches_numpy(T, sky, name, accel, kind):
    w, h = 128, 72
    limit = 64
    tp = dict(history_limit=limit, normal_threshold=0.9, depth_threshold=0.05)
    t = make(T, sky, name, w, h, accel=accel, denoise=dict(iterations=0), temporal=tp)
    t.options["camera_to_world"] = cam_at(0, kind)
    t.render(1)
    exempt_total, moved, flagged = 0, 0, 0.0
    for k in range(1, 5):
        hist = (t.clear_canvas(), t.read_denoise_history())[1]
        assert hist["valid"]
        t.update_scene(*t.scene)
        t.options["camera_to_world"] = cam_at(k, kind)
        t.options["time"] = 2000 + k
        argb = t.render(1).copy().reshape(h, w, 4)
        want = frame_ref(t, hist, **tp)
        got = t.read_denoised()
        t.clear_canvas()
        got_h = t.read_denoise_history()
        got_count = got_h["count"]
        border = want["rep"]["borderline"]
        with np.errstate(all="ignore"):
            ok = np.isclose(got[..., :3], want["c"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= np.isclose(got[..., 3], want["V"], rtol=1e-4, atol=1e-7, equal_nan=True)
            ok &= np.isclose(got_count, want["commit"]["count"], rtol=1e-4)
            ok &= (np.abs(argb.astype(int) - D.tonemap(want["c"]).astype(int)) <= 1).all(-1)
        bad = ~ok & ~border
        assert not bad.any(), (k, np.argwhere(bad)[:5])
        # and bit for bit where the restatement does not flag the pixel (tests/test_gpu_denoise_temporal_cases.py's rule)
        exact, _, _ = TC.compare_setup(want, got, argb, got_h)
        assert not (~exact & ~border).any(), (k, np.argwhere(~exact & ~border)[:5])
        # flagged pixels are exempt only where they differ: a translation leaves the far field (parallax -> 0) within 1e-4 of
        # whole-pixel coordinates, which flags up to ~0.5 % of the pixels, nearly all of them computed alike
        exempt = int((~ok & border).sum())
        assert exempt < 1e-3 * w * h, (k, exempt)
        exempt_total += exempt
        flagged = max(flagged, float(border.mean()))
        # disoccluded (no tap the reference counts): no history on the GPU either
        dis = (want["cur"]["cov"] > 0) & (want["rep"]["taps"] == 0) & ~border
        assert dis.any() and np.all(got_count[dis] == want["cur"]["P"])
        moved += int((want["h"] > 0).sum())
        # the history was put back for the next frame by the clear above; the next loop clears nothing traced
    assert moved > 0
    print(f"{name}/{kind}: {exempt_total} borderline pixels differed; at most {flagged * 100:.2f}% of a frame's pixels flagged")
    t.close()


# ---- 5. what drops the history ----------------------------------------------------------------------------------------------
def test_drop_rules(T, sky):
    w, h = 48, 32
    t = make(T, sky, "spheres", w, h, denoise={}, temporal={})
    shapes, tris, mats = t.scene

    def commit():
        t.options["time"] += 1
        t.render(1)
        t.clear_canvas()
        assert t.read_denoise_history()["valid"]

    def valid():
        return t.read_denoise_history()["valid"]

    commit()
    before = t.read_denoise_history()
    t.clear_canvas()  # nothing traced: the history stays
    after = t.read_denoise_history()
    check_commit(after, before)
    same = [np.frombuffer(bytearray(a.tobytes()), a.dtype) for a in (shapes, tris, mats)]  # new arrays, the same bytes (padding too)
    t.update_scene(*same)
    assert valid()
    t.set_denoise(sigma_luminance=2.0)  # not a clearing change
    assert valid()
    t.set_denoise_temporal(history_limit=8)  # on -> on with other settings
    assert valid()
    triggers = [
        lambda: t.reset_denoise_history(),
        lambda: (t.set_denoise_temporal(False), t.set_denoise_temporal()),
        lambda: (t.set_denoise(False), t.set_denoise(), t.set_denoise_temporal()),
        lambda: t.set_denoise(feature_samples=2),
        lambda: t.set_skybox(sky),
    ]
    moved = shapes.copy()
    moved["sphere_position"][0, 0] += 0.25
    edited = mats.copy()
    edited[0]["smoothness"] = 0.5
    triggers += [lambda: t.update_scene(moved, tris, mats), lambda: t.update_scene(shapes, tris, edited)]
    sd = t.scene_data.copy()
    triggers += [lambda: (t.scene_data.__setitem__("sun_intensity", 2.0), t.update_scene(shapes, tris, mats))]
    for i, trig in enumerate(triggers):
        commit()
        trig()
        assert not valid(), i
        t.update_scene(shapes, tris, mats)
    t.scene_data = sd
    t.close()


def test_set_denoise_off_turns_temporal_off(T, sky):
    t = make(T, sky, "spheres", 48, 32, denoise={}, temporal={})
    t.set_denoise(False)
    t.set_denoise()
    spatial = make(T, sky, "spheres", 48, 32, denoise={})
    for k in range(2):
        assert np.array_equal(next_frame(t, k, "move", 60 + k), next_frame(spatial, k, "move", 60 + k))
    t.close()
    spatial.close()


# ---- 6. quality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 1)])
def test_quality_moving_camera(T, sky, name, accel):
    w, h, frames = 160, 90, 8
    last = cam_at(frames - 1, "move")
    g = make(T, sky, name, w, h, spp=4096, accel=accel, time=4242)
    g.options["camera_to_world"] = last
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    sp = make(T, sky, name, w, h, accel=accel, denoise={})
    tm = make(T, sky, name, w, h, accel=accel, denoise={}, temporal={})
    for k in range(frames):
        for t in (sp, tm):
            next_frame(t, k, "move", 900 + k)
    a, b = sp.read_denoised()[..., :3], tm.read_denoised()[..., :3]
    tm.clear_canvas()
    hist = tm.read_denoise_history()
    dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)  # a first hit, and no history reached it
    mse_s = float(np.mean((tone(a) - ref) ** 2))
    mse_t = float(np.mean((tone(b) - ref) ** 2))
    dis_s = float(np.mean((tone(a)[dis] - ref[dis]) ** 2))
    dis_t = float(np.mean((tone(b)[dis] - ref[dis]) ** 2))
    print(f"{name}: spatial MSE {mse_s:.3e}, temporal {mse_t:.3e} ({mse_t / mse_s:.3f}); disoccluded {dis.mean() * 100:.1f}% of pixels, "
          f"{dis_t / dis_s:.3f}")
    assert mse_t <= 0.7 * mse_s
    assert dis.any() and dis_t <= 1.25 * dis_s
    # the camera stops: the front-end goes on at 2 spp without a clear to 1024 samples; the history weighs no more than
    # history_limit of them
    for t in (sp, tm):
        for i in range(1, 512):
            t.options["time"] = 7000 + i
            if i < 511:
                t.trace()
            else:
                t.render(i + 1)  # the front-end's ticks: the dispatches since the last clear
    p = D.psnr(tone(tm.read_denoised()[..., :3]), tone(sp.read_denoised()[..., :3]))
    print(f"{name}: after the camera stopped, temporal vs spatial at 1024 spp: {p:.1f} dB")
    assert p >= 40.0
    sp.close()
    tm.close()


# ---- 7. render paths, determinism, srt_headless ---------------------------------------------------------------------------
def test_render_paths_and_determinism(T, sky):
    w, h = 96, 64
    ts = [make(T, sky, "mixed", w, h, denoise={}, temporal={}) for _ in range(5)]
    blk, blk2, asy, pip, res = ts
    buf = np.zeros(w * h * 4, np.uint8)
    want, got = [], {"async": [], "resolve": [], "again": []}
    piped = {}
    for k in range(4):
        for t in ts:
            t.clear_canvas()
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(k, "yaw")
            t.options["time"] = 80 + k
        want.append(blk.render(1).copy())
        got["again"].append(blk2.render(1).copy())
        o = np.zeros(w * h * 4, np.uint8)
        asy.render_async(1, o)
        asy.synchronize()
        got["async"].append(o)
        res.trace()
        res.resolve_denoised(1)
        res.synchronize()
        got["resolve"].append(res.read_argb().copy())
        n = pip.render_pipelined(1, buf)
        if n >= 0:
            piped[n] = buf.copy()
    n = pip.pipeline_flush(buf)
    piped[n] = buf.copy()
    for k in range(4):
        for key, v in got.items():
            assert np.array_equal(want[k], v[k].reshape(want[k].shape)), (key, k)
        assert np.array_equal(want[k], piped[k]), ("pipelined", k)
    assert bits_equal(blk.read_denoised(), blk2.read_denoised())
    for t in ts:
        t.close()


def test_headless_temporal_move_replays(T, sky, tmp_path):
    from simple_raytracer_amd import build
    exe = build.build_headless()
    pre = tmp_path / "m"
    w, h, frames, dx = 64, 48, 4, 0.02
    subprocess.run([str(exe), "--scene", "spheres", "--width", str(w), "--height", str(h), "--spp", "2", "--frames", str(frames), "--denoise", "5",
                    "--temporal", "--move", str(dx), "--dump", str(pre)], check=True, timeout=120)
    rd = np.fromfile(f"{pre}.rd.bin", R.RENDER_DATA).reshape(())
    sd = np.fromfile(f"{pre}.sd.bin", R.SCENE_DATA).reshape(())
    shapes = np.fromfile(f"{pre}.shapes.bin", R.SHAPE)
    tris = np.fromfile(f"{pre}.tris.bin", R.TRIANGLE)
    mats = np.fromfile(f"{pre}.mats.bin", R.MATERIAL)
    sky_h = np.fromfile(f"{pre}.sky.bin", np.float32).reshape(1024, 2048, 4)
    want = np.fromfile(f"{pre}.argb.bin", np.uint8)
    t = T.Tracer(w, h)
    t.set_skybox(sky_h)
    t.set_denoise(iterations=5)
    t.set_denoise_temporal()
    t.scene_data = sd.copy()
    t.scene_data["num_shapes"] = 0  # as Tracer::update_scene before its first call
    out = None
    for f in range(frames):
        t.clear_canvas()
        t.update_scene(shapes, tris, mats)
        o = rd.copy()
        cam = np.array(rd["camera_to_world"], np.float32)
        cam[3][0] = np.float32(dx) * np.float32(f)
        o["camera_to_world"] = cam
        o["time"] = np.uint32((int(rd["time"]) - 7919 * (frames - 1 - f)) & 0xFFFFFFFF)
        t.options = o
        out = t.render(1)
    assert np.array_equal(out, want)
    t.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def test_error_codes(T, sky):
    lib = T.load_library()
    t = make(T, sky, "spheres", 64, 48, spp=1)
    d = T.TemporalParams()
    assert lib.srt_temporal_defaults(C.byref(d)) == 0 and lib.srt_temporal_defaults(None) == 1
    assert lib.srt_read_denoise_history(t._h, None, None, None, None, None) == 3  # never enabled
    assert lib.srt_set_denoise_temporal(t._h, C.byref(d)) == 3  # the denoiser is off
    assert lib.srt_set_denoise_temporal(t._h, None) == 0
    t.set_denoise()
    for field, bad in [("history_limit", 0), ("history_limit", (1 << 20) + 1), ("normal_threshold", 1.5), ("normal_threshold", float("nan")),
                       ("depth_threshold", 0.0), ("depth_threshold", float("inf")), ("depth_threshold", -0.1)]:
        e = T.TemporalParams.from_buffer_copy(d)
        setattr(e, field, bad)
        assert lib.srt_set_denoise_temporal(t._h, C.byref(e)) == 1, field
    e = T.TemporalParams.from_buffer_copy(d)
    e.reserved[2] = 1
    assert lib.srt_set_denoise_temporal(t._h, C.byref(e)) == 1
    e = T.TemporalParams.from_buffer_copy(d)
    e.history_limit, e.normal_threshold = 1 << 20, -1.0
    assert lib.srt_set_denoise_temporal(t._h, C.byref(e)) == 0
    assert lib.srt_set_denoise_temporal(t._h, C.byref(d)) == 0
    valid = C.c_int(7)
    assert lib.srt_read_denoise_history(t._h, None, None, None, None, C.byref(valid)) == 0 and valid.value == 0
    assert lib.srt_set_partition(t._h, 0, 2, 8) == 3
    assert lib.srt_reset_denoise_history(t._h) == 0 and lib.srt_reset_denoise_history(None) == 1
    assert lib.srt_set_denoise_temporal(None, C.byref(d)) == 1
    assert lib.srt_read_denoise_history(None, None, None, None, None, None) == 1
    off = T.TemporalParams.from_buffer_copy(d)
    off.enable = 0
    assert lib.srt_set_denoise_temporal(t._h, C.byref(off)) == 0
    lib.srt_set_denoise(t._h, None)
    assert lib.srt_set_partition(t._h, 0, 2, 8) == 0
    t.set_denoise_temporal(False)
    t.close()
