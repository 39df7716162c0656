"""GPU: the edge-aware denoiser (srt_set_denoise): the primary-hit feature pass against the trace kernel's own
show_normals image, the moments reduction, the filter against its numpy restatement (tests/denoise_ref.py), identity,
quality, determinism, the render paths and the error codes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_ref as D
from conftest import bits_equal
from gpu_harness import T, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu


# ---- 1. feature pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 0), ("meshes", 1), ("mixed", 0), ("mixed", 1)])
def test_feature_normals_equal_show_normals(T, sky, name, accel):
    w, h = 96, 64
    t = make(T, sky, name, w, h, spp=1, accel=accel, denoise=dict(iterations=0), show_normals=True)
    t.render(1)
    canvas = t.read_canvas()
    inp = t.read_denoise_inputs()
    nd, ah = inp["normal_depth"], inp["albedo_hits"]
    hit = ah[..., 3] == 1.0
    assert set(np.unique(ah[..., 3])) <= {0.0, 1.0}
    assert hit.sum() > w * h // 10
    want = nd[..., :3] * np.float32(0.5) + np.float32(0.5)
    assert bits_equal(want[hit], canvas[..., :3][hit])
    assert np.all(nd[..., 3][hit] > 0) and np.all(nd[~hit] == 0)
    # every albedo is one material colour, or (1, 1, 1) where nothing was hit
    colors = {tuple(c) for c in scene(name)[2]["color"][:, :3].astype(np.float32).tolist()}
    assert np.all(ah[~hit][:, :3] == 1.0)
    assert all(tuple(c) in colors for c in ah[hit][:, :3].tolist())
    assert (inp["T"], inp["P"]) == (1, 1)
    t.close()


@pytest.mark.parametrize("name", ["meshes", "mixed"])
def test_feature_buffers_bvh_equal_scan(T, sky, name):
    out = []
    for accel in (0, 1):
        t = make(T, sky, name, 96, 64, spp=4, accel=accel, denoise=dict(feature_samples=3))
        t.render(1)
        out.append(t.read_denoise_inputs())
        t.close()
    for k in ("normal_depth", "albedo_hits"):
        assert np.array_equal(out[0][k].view(np.uint32), out[1][k].view(np.uint32)), k
    assert out[0]["albedo_hits"][..., 3].max() == 3.0


# ---- 2. moments -----------------------------------------------------------------------------------------------------------
def test_moments_of_one_sample(T, sky):
    t = make(T, sky, "mixed", 96, 64, spp=1, denoise={})
    t.render(1)
    canvas = t.read_canvas()
    m = t.read_denoise_inputs()["moments"]
    want = D.lum(canvas[..., :3]) ** 2
    ok = np.isfinite(want)
    ulp = np.abs(m.view(np.int32)[ok].astype(np.int64) - want.astype(np.float32).view(np.int32)[ok].astype(np.int64))
    assert ulp.max() <= 1
    t.close()


def test_counts_and_batched_moments(T, sky):
    w, h = 64, 48
    a = make(T, sky, "mixed", w, h, spp=1, denoise={})
    b = make(T, sky, "mixed", w, h, spp=1, denoise={})
    b.set_radiance_budget(w * h * 12 * 2)  # sample batches: the moments are carried across them
    for i, ns in enumerate((1, 6, 3, 8)):
        for t in (a, b):
            t.options["num_samples"] = ns
            t.options["time"] = 100 + i
            t.render(i + 1)
    ia, ib = a.read_denoise_inputs(), b.read_denoise_inputs()
    assert (ia["T"], ia["P"]) == (4, 18) and (ib["T"], ib["P"]) == (4, 18)
    assert b.last_trace_launches()[0] > 1  # the last dispatch ran in several sample batches
    for k in ("moments", "normal_depth", "albedo_hits"):
        assert bits_equal(ia[k], ib[k]), k
    assert bits_equal(a.read_canvas(), b.read_canvas())
    a.close()
    b.close()


def test_canvas_unchanged_by_the_denoiser(T, sky):
    off = make(T, sky, "mixed", 96, 64, spp=4)
    on = make(T, sky, "mixed", 96, 64, spp=4, denoise={})
    for i in range(3):
        for t in (off, on):
            t.options["time"] = 50 + i
            t.render(i + 1)
    assert bits_equal(off.read_canvas(), on.read_canvas())
    off.close()
    on.close()


# ---- 3. filter against numpy, 4. identity --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "meshes"])
def test_filter_matches_numpy(T, sky, name):
    t = make(T, sky, name, 96, 64, spp=4, accel=1, denoise=dict(feature_samples=2))
    for i in range(2):
        t.options["time"] = 900 + i
        argb = t.render(i + 1).reshape(64, 96, 4)
    inp = t.read_denoise_inputs()
    got = t.read_denoised()
    F = 2 * min(2, 4)  # two dispatches of min(feature_samples, num_samples) feature rays
    hdr, want_argb = D.denoise(t.read_canvas(), inp["normal_depth"], inp["albedo_hits"], inp["moments"], inp["T"], inp["P"], F, 2)
    np.testing.assert_allclose(got[..., :3], hdr[..., :3], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got[..., 3], hdr[..., 3], rtol=1e-3, atol=1e-9)
    assert np.abs(argb.astype(int) - want_argb.astype(int)).max() <= 1
    t.close()


FILTER_FRAMES = [(96, 64), (37, 29), (17, 16), (1, 33), (33, 1), (130, 5)]  # tiles of 16x16: whole, ragged, one column or row
FILTER_KS = (1, 2, 3, 4, 5, 8)  # odd and even K end in either ping-pong buffer; 8: steps up to 128, beyond every frame here
FILTER_SIGMAS = {
    "default": {},
    "tight": dict(sigma_luminance=0.5, sigma_normal=16.0, sigma_depth=0.1, sigma_albedo=0.5),
    "loose": dict(sigma_luminance=64.0, sigma_normal=1.0, sigma_depth=10.0, sigma_albedo=2.0),
    # the small end of each sigma; sigma_albedo = 1e-20: 1 / sigma^2 is beyond float's range (the library clamps it)
    "small_l": dict(sigma_luminance=1e-20),
    "small_n": dict(sigma_normal=1e-20),
    "small_z": dict(sigma_depth=1e-20),
    "small_a": dict(sigma_albedo=1e-20),
}
FILTER_DISPATCHES = ((4, 900), (1, 4096), (3, 901))  # (num_samples, time)


def check_filter(got_hdr, got_argb, want_hdr, want_argb, what):
    np.testing.assert_allclose(got_hdr[..., :3], want_hdr[..., :3], rtol=1e-4, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(got_hdr[..., 3], want_hdr[..., 3], rtol=1e-3, atol=1e-9, err_msg=what)
    assert np.abs(got_argb.astype(int) - want_argb.astype(int)).max() <= 1, what


def filter_against_numpy(t, sigmas, fs, k_render, what):
    """Dispatches through render() with k_render passes, then every K of FILTER_KS by srt_set_denoise (the same
    feature_samples: the sums stay) and srt_resolve_denoised with a ticks value that is not the dispatch count."""
    h, w = t.height, t.width
    F = 0
    for i, (ns, tm) in enumerate(FILTER_DISPATCHES):
        t.options["num_samples"] = ns
        t.options["time"] = tm
        argb = t.render(i + 1).reshape(h, w, 4)
        F += min(fs, ns)
    inp = t.read_denoise_inputs()
    canvas = t.read_canvas()
    args = (canvas, inp["normal_depth"], inp["albedo_hits"], inp["moments"], inp["T"], inp["P"], F)
    steps = D.denoise_steps(*args, len(FILTER_DISPATCHES), k_render, **sigmas)
    check_filter(t.read_denoised(), argb, *steps[k_render], f"{what} render K={k_render}")
    ticks = 7
    steps = D.denoise_steps(*args, ticks, max(FILTER_KS), **sigmas)
    for K in FILTER_KS:
        t.set_denoise(feature_samples=fs, iterations=K, **sigmas)
        t.resolve_denoised(ticks)
        t.synchronize()
        check_filter(t.read_denoised(), t.read_argb(), *steps[K], f"{what} K={K}")
    assert t.read_denoise_inputs()["T"] == len(FILTER_DISPATCHES)
    return canvas


@pytest.mark.parametrize("sig", sorted(FILTER_SIGMAS))
@pytest.mark.parametrize("w,h", FILTER_FRAMES)
def test_filter_matrix_matches_numpy(T, sky, w, h, sig):
    """The filter against numpy over frame shapes, K and sigma sets, with F counted from the dispatches."""
    k_render = FILTER_KS[(FILTER_FRAMES.index((w, h)) + sorted(FILTER_SIGMAS).index(sig)) % len(FILTER_KS)]
    sigmas = FILTER_SIGMAS[sig]
    t = make(T, sky, "mixed", w, h, spp=4, accel=1, denoise=dict(feature_samples=2, iterations=k_render, **sigmas))
    filter_against_numpy(t, sigmas, 2, k_render, f"{w}x{h} {sig}")
    t.close()


def test_filter_skips_non_finite_pixels(T, sky):
    """A material with a NaN and an inf colour: NaN and inf pixels are neither filtered nor taps, on both sides."""
    shapes, tris, mats = S.sphere_scene()
    mats = mats.copy()
    mats["color"][2] = (np.nan, 0.5, np.inf)
    w, h = 48, 40
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.set_acceleration(1)
    t.options = R.render_data(w, h, 4, 10, camera_to_world=S.default_camera(), time=1)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.set_denoise(feature_samples=3, iterations=4)
    canvas = filter_against_numpy(t, {}, 3, 4, "non-finite")
    bad = ~np.all(np.isfinite(canvas[..., :3]), axis=-1)
    assert bad.any() and not bad.all()
    t.close()


def test_zero_iterations_is_plain_render(T, sky):
    off = make(T, sky, "mixed", 96, 64, spp=4)
    on = make(T, sky, "mixed", 96, 64, spp=4, denoise=dict(iterations=0))
    for i in range(3):
        outs = []
        for t in (off, on):
            t.options["time"] = 60 + i
            outs.append(t.render(i + 1))
        assert np.array_equal(outs[0], outs[1])
    off.close()
    on.close()


# ---- 5. quality, 6. preservation ----------------------------------------------------------------------------------------
def ground_truth(T, sky, name, w, h, accel):
    t = make(T, sky, name, w, h, spp=4096, accel=accel, denoise={}, time=4242)
    t.render(1)
    canvas = t.read_canvas()
    preserved = t.read_denoised()
    t.close()
    return canvas[..., :3], preserved[..., :3]


@pytest.mark.parametrize("name,accel", [("spheres", 0), ("meshes", 1)])
def test_quality_and_preservation(T, sky, name, accel):
    w, h = 160, 90
    gt, gt_filtered = ground_truth(T, sky, name, w, h, accel)
    t = make(T, sky, name, w, h, spp=4, accel=accel, denoise={}, time=31)
    t.render(1)
    noisy = t.read_canvas()[..., :3]
    den = t.read_denoised()[..., :3]
    ref = tone(gt)
    mse_noisy = float(np.mean((tone(noisy) - ref) ** 2))
    mse_den = float(np.mean((tone(den) - ref) ** 2))
    print(f"{name}: noisy MSE {mse_noisy:.3e}, denoised {mse_den:.3e} ({mse_den / mse_noisy:.3f}); "
          f"converged image through the filter: {D.psnr(tone(gt_filtered), ref):.1f} dB")
    assert mse_den <= 0.5 * mse_noisy
    assert D.psnr(tone(gt_filtered), ref) >= 40.0
    t.close()


# ---- 7. determinism and paths --------------------------------------------------------------------------------------------
def test_two_denoises_identical(T, sky):
    t = make(T, sky, "mixed", 96, 64, spp=4, denoise={})
    t.render(1)
    a, ha = t.read_argb().copy(), t.read_denoised()
    t.resolve_denoised(1)
    t.synchronize()
    b, hb = t.read_argb(), t.read_denoised()
    assert np.array_equal(a, b) and np.array_equal(ha.view(np.uint32), hb.view(np.uint32))
    t.close()


def test_async_and_pipelined_equal_blocking(T, sky):
    w, h = 96, 64
    blk, asy, pip = (make(T, sky, "mixed", w, h, spp=2, denoise={}) for _ in range(3))
    want, got_async, got_pipe = [], [], {}
    buf = np.zeros(w * h * 4, np.uint8)
    for i in range(4):
        for t in (blk, asy, pip):
            t.options["time"] = 70 + i
        want.append(blk.render(i + 1).copy())
        o = np.zeros(w * h * 4, np.uint8)
        asy.render_async(i + 1, o)
        asy.synchronize()
        got_async.append(o)
        n = pip.render_pipelined(i + 1, buf)
        if n >= 0:
            got_pipe[n] = buf.copy()
    n = pip.pipeline_flush(buf)
    got_pipe[n] = buf.copy()
    for i in range(4):
        assert np.array_equal(want[i], got_async[i]), i
        assert np.array_equal(want[i], got_pipe[i]), i
    for t in (blk, asy, pip):
        t.close()


def test_enable_then_disable_equals_fresh(T, sky):
    fresh = make(T, sky, "mixed", 96, 64, spp=2)
    used = make(T, sky, "mixed", 96, 64, spp=2, denoise={})
    used.render(1)
    used.set_denoise(False)
    used.clear_canvas()
    for i in range(2):
        for t in (fresh, used):
            t.options["time"] = 80 + i
        assert np.array_equal(fresh.render(i + 1), used.render(i + 1))
    assert bits_equal(fresh.read_canvas(), used.read_canvas())
    fresh.close()
    used.close()


def test_headless_denoise_writes_ppm(tmp_path):
    from simple_raytracer_amd import build
    exe = build.build_headless()
    out = tmp_path / "d.ppm"
    subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", "2", "--denoise", "5",
                    "--out", str(out)], check=True, timeout=120)
    data = out.read_bytes()
    assert data.startswith(b"P6") and len(data) > 64 * 48 * 3


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def test_error_codes(T, sky):
    lib = T.load_library()
    t = make(T, sky, "spheres", 64, 48, spp=1)
    d = T.DenoiseParams()
    lib.srt_denoise_defaults(C.byref(d))
    assert lib.srt_resolve_denoised(t._h, 1) == 3  # off
    for field, bad in [("iterations", -1), ("iterations", 9), ("feature_samples", 0), ("feature_samples", 65), ("sigma_luminance", 0.0),
                       ("sigma_normal", -1.0), ("sigma_depth", float("nan")), ("sigma_albedo", float("inf")), ("reserved", 1)]:
        e = T.DenoiseParams.from_buffer_copy(d)
        setattr(e, field, bad)
        assert lib.srt_set_denoise(t._h, C.byref(e)) == 1, field
    assert lib.srt_set_denoise(t._h, C.byref(d)) == 0
    assert lib.srt_resolve_denoised(t._h, 1) == 3  # nothing traced since the clear
    assert lib.srt_set_partition(t._h, 0, 2, 8) == 3
    assert lib.srt_set_denoise(t._h, None) == 0
    assert lib.srt_set_partition(t._h, 0, 2, 8) == 0
    assert lib.srt_set_denoise(t._h, C.byref(d)) == 3
    off = T.DenoiseParams.from_buffer_copy(d)
    off.enable = 0
    assert lib.srt_set_denoise(t._h, C.byref(off)) == 0
    t.close()
