"""GPU: albedo demodulation for the denoiser (srt_set_denoise_demodulation). The filter against its numpy
restatement (tests/demod_ref.py) on textured scenes at §10's tolerances, K = 0, off-is-off and determinism, the switch's
rules, the filter after the temporal and the moved set-up, a device group against the single handle, and quality: on a
noise-textured scene against the colour filter of the same build, on untextured scenes against test_gpu_denoise.py's thresholds."""
import numpy as np
import pytest

import demod_ref as DM
import denoise_ref as D
import temporal_ref as TR
from conftest import bits_equal
from gpu_harness import T, cam_at, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
SRT_ERR_STATE = 3


def case(kind):
    """-> shapes, tris, mats, textures, bindings, uvs, accel"""
    if kind == "noise":
        return (*S.textured_noise_scene(), None, 0)
    if kind == "mesh":  # the two-mesh scene, every material textured, planar UVs, under the BVH
        return (*S.textured_mesh_scene(), 1)
    if kind == "eps":  # texels (0, 0, 0) and (1, 0, 0): every channel of some pixel is below SRT_DEMOD_EPS
        shapes, tris, mats, _, bindings = S.textured_noise_scene()
        return shapes, tris, mats, [S.checker_texture(2, 2, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))], bindings, None, 0
    if kind == "nonfinite":  # test_gpu_denoise.py's means, materials: a NaN colour on the small sphere (unbound) gives NaN pixels; an inf
        # colour gives NaN too (the mask's mix(colour, 1, 0) is 0 * inf), so the inf pixels come from a small emitter of infinite strength
        shapes, tris, mats, textures, bindings = S.textured_noise_scene()
        mats = R.concat(R.MATERIAL, mats, np.array([R.material((1, 1, 1), emission=(1.0, 1.0, 1.0), emission_strength=np.inf)], R.MATERIAL))
        mats["color"][2] = (np.nan, 0.5, np.inf)
        shapes = R.concat(R.SHAPE, shapes, np.array([R.sphere(3, (0.2, 1.7, -1.0), 0.25)], R.SHAPE))
        b = np.zeros(4, R.MATERIAL_TEXTURE)
        b[:3] = bindings
        b[2] = b[3] = R.material_texture()
        return shapes, tris, mats, textures, b, None, 0
    if kind in ("spheres", "meshes"):  # untextured: gpu_harness.scene
        return (*scene(kind), None, None, None, 1 if kind == "meshes" else 0)
    raise ValueError(kind)


def tracer(T, sky, kind, w, h, spp=4, fs=None, K=5, time=31, cam=None, temporal=None, motion=False, demod=True, group=0, rpb=8):
    """gpu_harness.make over case(kind) with its textures bound, the denoiser on with feature_samples = fs (None: spp) and the
    demodulation switch as given; group > 0: a TracerGroup of that many virtual devices."""
    shapes, tris, mats, textures, bindings, uvs, accel = case(kind)
    dn = dict(iterations=K, feature_samples=min(spp, 64) if fs is None else fs)
    if group:
        t = T.TracerGroup(w, h, n_devices=group, devices=[0] * group, rows_per_block=rpb)
        t.set_skybox(sky)
        t.set_acceleration(accel)
        t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera() if cam is None else cam, time=time)
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        t.set_denoise(**dn)
        t.scene = (shapes, tris, mats)
    else:
        t = make(T, sky, (shapes, tris, mats), w, h, spp=spp, accel=accel, time=time, cam=cam, denoise=dn, temporal=temporal, motion=motion)
    if textures is not None:
        t.set_textures(textures)
        t.set_material_textures(bindings)
        t.set_triangle_uvs(uvs)
    t.clear_canvas()
    if demod:
        t.set_denoise_demodulation(True)
    return t


def check_filter(got_hdr, got_argb, want_hdr, want_argb, what):
    """§10's tolerances (tests/test_gpu_denoise.py check_filter)"""
    np.testing.assert_allclose(got_hdr[..., :3], want_hdr[..., :3], rtol=1e-4, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(got_hdr[..., 3], want_hdr[..., 3], rtol=1e-3, atol=1e-9, err_msg=what)
    assert np.abs(got_argb.astype(int) - want_argb.astype(int)).max() <= 1, what


# ---- 1. the filter against numpy -----------------------------------------------------------------------------------------
# 33x17: ragged, smaller than two blocks, steps 4-16 leave the image; 64x48: whole blocks; 160x90: the quality tests' frame
FRAMES = [(33, 17), (64, 48), (160, 90)]
KS = (1, 2, 5, 8)  # odd and even K end in either ping-pong image; 8: steps beyond every frame here
DISPATCHES = ((4, 900), (3, 901))  # (num_samples, time)


@pytest.mark.parametrize("kind,w,h", [(k, w, h) for k in ("noise", "mesh", "eps") for w, h in FRAMES] + [("nonfinite", 48, 40)])
def test_filter_matches_numpy(T, sky, kind, w, h):
    """Inputs are the handle's own; the frame is rendered with K = 5 and then filtered again for every K of KS with a ticks
    value that is not the dispatch count (tests/test_gpu_denoise.py filter_against_numpy, with the switch on)."""
    fs = 4
    t = tracer(T, sky, kind, w, h, fs=fs, K=5)
    F = 0
    for i, (ns, tm) in enumerate(DISPATCHES):
        t.options["num_samples"] = ns
        t.options["time"] = tm
        argb = t.render(i + 1).reshape(h, w, 4)
        F += min(fs, ns)
    assert t.last_filter_demodulated() and (t.last_trace_textured() or kind in ("spheres", "meshes"))
    inp, canvas = t.read_denoise_inputs(), t.read_canvas()
    args = (canvas, inp["normal_depth"], inp["albedo_hits"], inp["moments"], inp["T"], inp["P"], F)
    check_filter(t.read_denoised(), argb, *DM.denoise(*args, len(DISPATCHES), 5), f"{kind} {w}x{h} render")
    ticks = 7
    steps = DM.denoise_steps(*args, ticks, max(KS))
    for K in KS:
        t.set_denoise(feature_samples=fs, iterations=K)
        t.resolve_denoised(ticks)
        t.synchronize()
        check_filter(t.read_denoised(), t.read_argb().reshape(h, w, 4), *steps[K], f"{kind} {w}x{h} K={K}")
    A = inp["albedo_hits"][..., :3] / np.float32(F)
    hit = inp["albedo_hits"][..., 3] > 0
    if kind == "eps":  # the clamp is exercised: pixels whose three channels are all below SRT_DEMOD_EPS, and (1, 0, 0) ones
        assert (hit & np.all(A < DM.EPS, axis=-1)).any() and (hit & (A[..., 0] == 1) & (A[..., 1] == 0)).any()
    if kind == "nonfinite":
        bad = ~np.all(np.isfinite(canvas[..., :3]), axis=-1)
        assert np.isnan(canvas[..., 0]).any() and np.isinf(canvas[..., 2]).any() and not bad.all()
        got = t.read_denoised()
        assert bits_equal(got[bad][:, :3], (canvas[bad][:, :3] / np.float32(ticks)))  # neither filtered nor divided
        assert np.all(np.isfinite(got[~bad]))  # and no tap
    t.close()


# ---- 2. K = 0, 3. off is off, determinism ---------------------------------------------------------------------------------
def test_zero_iterations_is_the_plain_resolve(T, sky):
    w, h = 64, 48
    plain = tracer(T, sky, "noise", w, h, K=0, demod=False)
    plain.set_denoise(False)
    plain.clear_canvas()
    on = tracer(T, sky, "noise", w, h, K=0)
    for i in range(2):
        for t in (plain, on):
            t.options["time"] = 60 + i
        assert np.array_equal(plain.render(i + 1), on.render(i + 1)), i
        assert not on.last_filter_demodulated()
    on.set_denoise(feature_samples=4, iterations=1)
    on.resolve_denoised(2)
    assert on.last_filter_demodulated()
    on.set_denoise(feature_samples=4, iterations=0)
    on.resolve_denoised(2)
    on.synchronize()
    assert not on.last_filter_demodulated() and np.array_equal(on.read_argb(), plain.read_argb())
    plain.close()
    on.close()


def test_off_is_off_and_on_is_deterministic(T, sky):
    w, h = 64, 48
    never = tracer(T, sky, "noise", w, h, demod=False)
    toggled = tracer(T, sky, "noise", w, h, demod=True)
    on = never.render(1).copy(), toggled.render(1).copy()
    assert not never.last_filter_demodulated() and toggled.last_filter_demodulated()
    hdr_on = toggled.read_denoised()
    assert not np.array_equal(on[0], on[1])
    toggled.resolve_denoised(1)  # a second run with the switch on
    toggled.synchronize()
    assert np.array_equal(toggled.read_argb().ravel(), on[1]) and np.array_equal(toggled.read_denoised().view(np.uint32), hdr_on.view(np.uint32))
    toggled.set_denoise_demodulation(False)
    toggled.resolve_denoised(1)
    toggled.synchronize()
    assert not toggled.last_filter_demodulated()
    assert np.array_equal(toggled.read_argb().ravel(), on[0]) and bits_equal(toggled.read_denoised(), never.read_denoised())
    for t in (never, toggled):
        t.options["time"] = 32
    assert np.array_equal(never.render(2), toggled.render(2)) and bits_equal(never.read_denoised(), toggled.read_denoised())
    never.close()
    toggled.close()


# ---- 4. errors and coupling ------------------------------------------------------------------------------------------------
def test_errors_and_coupling(T, sky):
    lib = T.load_library()
    w, h = 48, 32
    t = make(T, sky, "spheres", w, h)
    assert lib.srt_set_denoise_demodulation(t._h, 1) == SRT_ERR_STATE  # the denoiser is off
    assert lib.srt_set_denoise_demodulation(t._h, 0) == 0
    t.set_denoise()
    t.set_denoise_temporal()
    t.set_denoise_demodulation(True)
    t.render(1)
    assert t.last_filter_demodulated()
    t.clear_canvas()  # the commit: the frame becomes the history
    before = t.read_denoise_history()
    assert before["valid"]
    t.set_denoise_demodulation(False)
    t.set_denoise_demodulation(True)
    after = t.read_denoise_history()
    assert after["valid"]
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(before[k], after[k]), k
    t.set_denoise(sigma_luminance=2.0)  # another setting of the denoiser: the switch stays
    t.render(1)
    assert t.last_filter_demodulated()
    t.set_denoise(False)  # turning the denoiser off turns it off
    t.set_denoise()
    t.render(1)
    assert not t.last_filter_demodulated()
    t.close()
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=8)
    assert lib.srt_group_set_denoise_demodulation(g._g, 1) == SRT_ERR_STATE
    with pytest.raises(T.SrtError):
        g.set_denoise_demodulation(True)
    assert not g.last_filter_demodulated()
    g.close()


# ---- 5. after the temporal set-up -----------------------------------------------------------------------------------------
def reach(K):
    return 2 * ((1 << K) - 1)  # how far a pixel's value travels in K passes


def near(mask, r):
    out = np.zeros_like(mask)
    for y, x in np.argwhere(mask):
        out[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return out


def test_with_temporal_reprojection_matches_numpy(T, sky):
    """Three frames of a moving camera, 2 spp: the demodulated result equals demod_ref applied to temporal_ref's set-up
    output. Where a history tap sits within float32 rounding of a threshold temporal_ref flags the pixel `borderline`, and
    the library may decide it the other way (tests/test_gpu_denoise_temporal.py): such a pixel's own set-up value, read
    with K = 0, is compared first, and the few that differ are left out together with the pixels their value reaches in
    K = 2 passes. Everything else is held to §10's tolerances."""
    w, h, K = 64, 48, 2
    tp = dict(history_limit=32, normal_threshold=0.9, depth_threshold=0.05)
    t = tracer(T, sky, "noise", w, h, spp=2, K=K, temporal=tp)
    t.options["camera_to_world"] = cam_at(0, "yaw")
    t.render(1)
    blended = 0
    for k in range(1, 4):
        t.clear_canvas()
        hist = t.read_denoise_history()
        assert hist["valid"]
        t.update_scene(*t.scene)
        t.options["camera_to_world"] = cam_at(k, "yaw")
        t.options["time"] = 2000 + k
        argb = t.render(1).copy().reshape(h, w, 4)
        assert t.last_filter_demodulated()
        got = t.read_denoised()
        inp = t.read_denoise_inputs()
        want = TR.temporal_setup(t.read_canvas(), inp, 2 * inp["T"], hist, t.options, **tp)  # F: two feature rays per dispatch
        t.set_denoise(feature_samples=2, iterations=0)  # the library's own set-up output
        t.resolve_denoised(1)
        setup = t.read_denoised()
        t.set_denoise(feature_samples=2, iterations=K)
        with np.errstate(all="ignore"):
            ok = np.isclose(setup[..., :3], want["c"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= np.isclose(setup[..., 3], want["V"], rtol=1e-4, atol=1e-7, equal_nan=True)
        differ = ~ok
        assert not (differ & ~want["rep"]["borderline"]).any(), k
        assert differ.sum() < 1e-3 * w * h, (k, int(differ.sum()))
        keep = ~near(differ, reach(K))
        cur = want["cur"]
        hdr, bytes_ = DM.filter_steps(want["c"], want["V"], cur["N"], cur["Z"], cur["A"], cur["cov"], iterations=K)[K]
        check_filter(got[keep], argb[keep], hdr[keep], bytes_[keep], f"frame {k}")
        blended += int((want["h"] > 0).sum())
    assert blended > 0.5 * w * h  # the history took part
    t.close()


def test_object_motion_with_nothing_moved_is_bit_equal(T, sky):
    """§12's rule carried over: object motion on and no shape moved is the frame without object motion, bit for bit."""
    w, h = 64, 48
    a = tracer(T, sky, "noise", w, h, spp=2, temporal={})
    b = tracer(T, sky, "noise", w, h, spp=2, temporal={}, motion=True)
    for k in range(3):
        outs = []
        for t in (a, b):
            t.clear_canvas()
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(k, "move")
            t.options["time"] = 300 + k
            outs.append(t.render(1).copy())
            assert t.last_filter_demodulated()
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(a.read_denoised(), b.read_denoised()), k
    assert a.read_denoise_history()["valid"] and b.read_denoise_history()["valid"]
    a.close()
    b.close()


# ---- 6. a device group -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_handle(T, sky, n):
    """§14's contract: the group's filtered frame, HDR and bytes, is the single device's bit for bit -- spatial, then with the
    temporal stage and a history."""
    w, h = 48, 40
    single = tracer(T, sky, "noise", w, h)
    group = tracer(T, sky, "noise", w, h, group=n, rpb=8)
    for k in range(3):
        if k == 1:
            for t in (single, group):
                t.set_denoise_temporal()
        outs = []
        for t in (single, group):
            t.clear_canvas()
            t.options["camera_to_world"] = cam_at(k, "yaw")
            t.options["time"] = 500 + k
            outs.append(t.render(1).copy())
            assert t.last_filter_demodulated()
        assert np.array_equal(outs[0], outs[1]), k
        assert np.array_equal(single.read_denoised().view(np.uint32), group.read_denoised().view(np.uint32)), k
    group.set_denoise_demodulation(False)
    single.set_denoise_demodulation(False)
    assert np.array_equal(single.render(2), group.render(2)) and not group.last_filter_demodulated()
    single.close()
    group.close()


@pytest.mark.parametrize("gpus", [1, 2])
def test_headless_demodulate_writes_a_textured_frame(tmp_path, gpus):
    """srt_headless --denoise 5 --demodulate on a textured scene, one device and a device group: a frame comes out, and it is
    not the frame without --demodulate."""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    img = np.random.default_rng(9).integers(0, 256, (16, 16, 3)).astype(np.uint8)
    ppm = tmp_path / "tex.ppm"
    ppm.write_bytes(b"P6\n16 16\n255\n" + img.tobytes())
    frames = []
    for extra in ([], ["--demodulate"]):
        out = tmp_path / f"f{len(extra)}.ppm"
        subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", "2", "--denoise", "5",
                        "--texture", str(ppm), "--texture-material", "0", "--texture-scale", "4", "--texture-nearest", "--gpus", str(gpus),
                        "--out", str(out)] + extra, check=True, timeout=120)
        frames.append(out.read_bytes())
    assert frames[1].startswith(b"P6") and len(frames[1]) > 64 * 48 * 3 and len(frames[0]) == len(frames[1])
    assert frames[0] != frames[1]


# ---- 7. quality ------------------------------------------------------------------------------------------------------------------
# Measured on an MI355X (160x90, 4 spp, feature_samples 4, default sigmas, tonemapped MSE against 4096 spp):
NOISE_QUALITY = dict(noisy=4.1438e-3, guided=3.0610e-3, demod=1.9571e-3, ratio=0.6393)  # the threshold is halfway between ratio and 1 (0.8197)
QW, QH = 160, 90


def quality(T, sky, kind):
    """-> tonemapped MSEs against a 4096-spp image of the same (textured) scene: the noisy 4-spp canvas, the colour-guided
    filter and the demodulated filter of the same canvas; and the PSNR of the converged image through the demodulated filter."""
    t = tracer(T, sky, kind, QW, QH, spp=4096, fs=4, time=4242)
    t.render(1)
    gt, gt_filtered = t.read_canvas()[..., :3], t.read_denoised()[..., :3]
    assert t.last_filter_demodulated()
    t.close()
    ref = tone(gt)
    t = tracer(T, sky, kind, QW, QH, spp=4, fs=4, time=31)
    t.render(1)
    noisy, demod = t.read_canvas()[..., :3], t.read_denoised()[..., :3]
    t.set_denoise_demodulation(False)
    t.resolve_denoised(1)
    guided = t.read_denoised()[..., :3]
    t.close()
    mse = lambda x: float(np.mean((tone(x) - ref) ** 2))
    out = dict(noisy=mse(noisy), guided=mse(guided), demod=mse(demod), psnr_converged=D.psnr(tone(gt_filtered), ref))
    out["ratio"] = out["demod"] / out["guided"]
    print(f"{kind}: noisy MSE {out['noisy']:.4e}, guided {out['guided']:.4e}, demodulated {out['demod']:.4e}, ratio {out['ratio']:.4f}; "
          f"converged image through the demodulated filter: {out['psnr_converged']:.1f} dB")
    return out


def test_noise_texture_quality(T, sky):
    """scenes.textured_noise_scene: the demodulated filter against the colour-guided filter of the same build (today's
    behaviour, which tests/test_gpu_denoise.py pins) on the same canvas."""
    q = quality(T, sky, "noise")
    assert q["demod"] < q["guided"]
    assert NOISE_QUALITY is not None, "the ratio has not been measured yet"
    assert q["ratio"] <= (NOISE_QUALITY["ratio"] + 1.0) / 2.0, q


@pytest.mark.parametrize("kind", ["spheres", "meshes"])
def test_untextured_quality_thresholds(T, sky, kind):
    """tests/test_gpu_denoise.py test_quality_and_preservation's scenes and thresholds with the switch on."""
    q = quality(T, sky, kind)
    assert q["demod"] <= 0.5 * q["noisy"]
    assert q["psnr_converged"] >= 40.0
