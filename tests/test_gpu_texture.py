"""GPU: albedo textures (include/srt_abi.h "albedo textures"), bit for bit: the switch, the first hit and the interfaces.
What a texel does at the SECOND and later hits of a path -- the whole canvas at full depth against the textured CPU oracle
(oracle/srt_oracle.c orc_render_textured) -- is tests/test_gpu_texture_paths.py's; the scenes, textures and the numpy route
to a first-hit texel that both share are tests/texture_cases.py. Here, by identities the untextured oracle expresses:
off means off; a texture of equal texels sampled NEAREST is exactly a colour (which runs the textured kernels over every
scene kind at full depth); the denoiser's albedo guide equals tests/texture_ref.py at the oracle's primary hits; a two-bounce
white scene's canvas equals texel(first hit) * the oracle's white radiance; partitions and groups reproduce the single
handle; each setter drops the temporal history."""
import numpy as np
import pytest

import denoise_ref as D
import golden_io
import temporal_ref
import texture_ref as TR
from conftest import bits_equal
from gpu_harness import SCENES, T, guide_scene, make, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S
from texture_cases import FIRST_HIT_CASES, TEXTURES, bind_all, constant_textures, first_hit_case, first_hit_texels, white_bindings, white_scene

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 29
GOLDEN = golden_io.load_cases()


def render_canvas(T, sky, scn, cam, accel, spp=4, bounces=10, textures=None, bindings=None, uvs=None, w=W, h=H, time=4242, budget=None):
    t = make(T, sky, scn, w, h, spp=spp, accel=accel, time=time, cam=cam)
    t.options["num_bounces"] = bounces
    if textures is not None:
        t.set_textures(textures)
    if bindings is not None:
        t.set_material_textures(bindings)
    if uvs is not None:
        t.set_triangle_uvs(uvs)
    if budget is not None:
        t.set_radiance_budget(budget)
    t.clear_canvas()
    t.render(1)
    out = t.read_canvas(), t.last_trace_textured(), t.options.copy(), t.scene_data.copy()
    t.close()
    return out


def oracle_canvas(oracle, sky, scn, rd, sd):
    shapes, tris, mats = scn
    return oracle.render(rd, sd, shapes, tris, mats, sky)


# ---- 4. off means off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", SCENES)
def test_off_means_off(T, sky, oracle, name, accel):
    """No texture bound -- nothing set at all, images uploaded but no material bound, every binding -1: the untextured
    kernels run and the canvas is the oracle's (what the committed goldens hold)."""
    shapes, tris, mats, cam = guide_scene(name)
    scn = (shapes, tris, mats)
    got0, tex0, rd, sd = render_canvas(T, sky, scn, cam, accel)
    want = oracle_canvas(oracle, sky, scn, rd, sd)
    assert not tex0 and bits_equal(got0, want)
    got1, tex1, _, _ = render_canvas(T, sky, scn, cam, accel, textures=[TR.checker(), TR.gradient()])
    assert not tex1 and bits_equal(got1, want)
    got2, tex2, _, _ = render_canvas(T, sky, scn, cam, accel, textures=[TR.checker()], bindings=bind_all(len(mats), lambda i: -1))
    assert not tex2 and bits_equal(got2, want)


# ---- 5. constant texture = colour --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_materials", [0, 80])  # 80 more 64-byte materials: the scene records no longer fit the LDS copy (USE_LDS false)
@pytest.mark.parametrize("side", [1, 4])
@pytest.mark.parametrize("name,accel", [s for s in SCENES if s[0] != "empty"])
def test_constant_texture_is_the_colour(T, sky, oracle, name, accel, side, pad_materials):
    """Every material bound, NEAREST, to a texture whose texels equal its colour: the textured kernels' canvas is the
    untextured oracle's bit for bit -- every scene kind, glass and metal included, scan and BVH, ten bounces."""
    shapes, tris, mats, cam = guide_scene(name)
    if pad_materials:
        mats = R.concat(R.MATERIAL, mats, np.zeros(pad_materials, R.MATERIAL))
    scn = (shapes, tris, mats)
    n_tex = min(len(mats), 64)
    textures = constant_textures(mats[:n_tex], side)
    bindings = bind_all(len(mats), lambda i: i if i < n_tex else -1, scale=(3.0, -2.5))
    got, textured, rd, sd = render_canvas(T, sky, scn, cam, accel, textures=textures, bindings=bindings)
    assert textured
    assert bits_equal(got, oracle_canvas(oracle, sky, scn, rd, sd)), (name, accel, side)


@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_committed_goldens_off_and_constant(T, sky, name, accel):
    """The committed goldens (tests/golden/cases.npz), frame sequence and all, array scan and BVH: with images uploaded but
    nothing bound the untextured kernels give the golden canvas and bytes; with every material on a 4x4 texture of its own
    colour, NEAREST, the textured kernels give them too."""
    g = GOLDEN[name]
    n_tex = min(len(g["mats"]), 64)
    for bound in (False, True):
        t = T.Tracer(int(g["rd"]["width"]), int(g["rd"]["height"]))
        t.set_skybox(sky)
        t.set_acceleration(accel)
        t.options = g["rd"].copy()
        t.scene_data = g["sd"].copy()
        t.set_textures(constant_textures(g["mats"][:n_tex], 4) if n_tex else [TR.checker()])
        if bound:
            t.set_material_textures(bind_all(len(g["mats"]), lambda i: i if i < n_tex else -1, scale=(7.0, 0.3)))
        t.update_scene(g["shapes"], g["tris"], g["mats"])
        t.clear_canvas()
        out = None
        for i, tm in enumerate(g["frames"]):
            t.options["time"] = np.uint32(tm)
            out = t.render(i + 1)
        canvas = t.read_canvas()
        assert t.last_trace_textured() == (bound and n_tex > 0 and not g["rd"]["show_normals"])
        assert bits_equal(canvas, g["canvas"]), (name, accel, bound)
        assert np.array_equal(out.reshape(g["argb"].shape), g["argb"])
        t.close()


def test_show_normals_ignores_textures(T, sky, oracle):
    shapes, tris, mats, cam = guide_scene("mixed")
    t = make(T, sky, (shapes, tris, mats), W, H, spp=2, cam=cam, show_normals=True)
    t.set_textures([TR.checker()])
    t.set_material_textures(bind_all(len(mats), lambda i: 0))
    t.clear_canvas()
    t.render(1)
    got = t.read_canvas()
    assert not t.last_trace_textured()
    assert bits_equal(got, oracle.render(t.options, t.scene_data, shapes, tris, mats, sky))
    t.close()


# ---- 6 / 7. the texel at the first hit (scenes, bindings and the numpy route: tests/texture_cases.py) ---------------------
@pytest.mark.parametrize("fs", [1, 3])
@pytest.mark.parametrize("filt", [TR.LINEAR, TR.NEAREST])
@pytest.mark.parametrize("kind,accel,with_uvs", FIRST_HIT_CASES)
def test_first_hit_albedo_is_the_texel(T, sky, oracle, kind, accel, with_uvs, filt, fs):
    """albedo_hits = the sum, in sample order, of texture_ref at the oracle's primary hits, bit for bit; normals, distances and
    hit counts are the untextured run's."""
    scn, bindings, uvs = first_hit_case(kind, filt, with_uvs)
    cam = S.default_camera()
    ns, results = 4, {}
    for textured in (False, True):
        t = make(T, sky, scn, W, H, spp=ns, accel=accel, time=99, cam=cam, denoise=dict(feature_samples=fs, iterations=0))
        if textured:
            t.set_textures(TEXTURES)
            t.set_material_textures(bindings)
            t.set_triangle_uvs(uvs)
            t.clear_canvas()
        t.render(1)
        results[textured] = t.read_denoise_inputs()
        rd, sd = t.options.copy(), t.scene_data.copy()
        assert t.last_trace_textured() == textured
        t.close()
    assert bits_equal(results[True]["normal_depth"], results[False]["normal_depth"])
    assert bits_equal(results[True]["albedo_hits"][..., 3], results[False]["albedo_hits"][..., 3])
    want = np.zeros((W * H, 3), F)
    for k in range(fs):
        tex, _ = first_hit_texels(oracle, rd, sd, scn, bindings, np.arange(W * H), np.full(W * H, k), uvs)
        want = (want + tex).astype(F)
    got = results[True]["albedo_hits"][..., :3].reshape(-1, 3)
    assert results[True]["albedo_hits"][..., 3].sum() > 0.5 * W * H * fs
    assert not bits_equal(got, results[False]["albedo_hits"][..., :3].reshape(-1, 3))
    assert bits_equal(got, want), (kind, accel, with_uvs, filt, fs, np.abs(got - want).max())


@pytest.mark.parametrize("w,h,budget_samples", [(W, H, None), (33, 7, 2)])  # a ragged frame in sample batches of 2
@pytest.mark.parametrize("filt", [TR.LINEAR, TR.NEAREST])
@pytest.mark.parametrize("kind,accel,with_uvs", FIRST_HIT_CASES)
def test_two_bounce_white_scene_is_texel_times_white_radiance(T, sky, oracle, kind, accel, with_uvs, filt, w, h, budget_samples):
    """num_bounces = 2, every material white, diffuse, without emission: a path's radiance is texel(first hit) * L_white, one
    float multiply per channel, L_white = the oracle's radiance of that path on the untextured scene (the second hit ends the
    path with emission 0; a miss adds mask * sky). Summed in the reduction's sample order, divided by the sample count."""
    scn, bindings, uvs = first_hit_case(kind, filt, with_uvs)
    shapes, tris, mats = scn
    ns = 8 if kind == "shapes" else 4
    got, textured, rd, sd = render_canvas(T, sky, scn, S.default_camera(), accel, spp=ns, bounces=2, textures=TEXTURES, bindings=bindings, uvs=uvs,
                                          w=w, h=h, budget=None if budget_samples is None else w * h * 12 * 2 * budget_samples)
    assert textured
    ids, smp = np.repeat(np.arange(w * h), ns), np.tile(np.arange(ns), w * h)
    L = oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, smp).astype(F)
    tex, hit = first_hit_texels(oracle, rd, sd, scn, bindings, ids, smp, uvs)
    rad = np.where(hit[:, None], (tex * L).astype(F), L).reshape(w * h, ns, 3)
    want = np.zeros((w * h, 3), F)
    for k in range(ns):
        want = (want + rad[:, k]).astype(F)
    want = (want / F(ns)).astype(F)
    assert bits_equal(got[..., :3].reshape(-1, 3), want), (kind, accel, with_uvs, filt, np.abs(got[..., :3].reshape(-1, 3) - want).max())


# ---- 8. deep paths, by identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_texture_on_an_unused_material_changes_nothing(T, sky, oracle, accel):
    shapes, tris, mats, cam = guide_scene("mixed")
    mats = R.concat(R.MATERIAL, mats, np.array([R.material(color=(0.3, 0.6, 0.9))], R.MATERIAL))
    scn = (shapes, tris, mats)
    got, textured, rd, sd = render_canvas(T, sky, scn, cam, accel, textures=[TR.checker()],
                                          bindings=bind_all(len(mats), lambda i: 0 if i == len(mats) - 1 else -1, filt=TR.LINEAR))
    assert textured  # (the textured kernels run: a material of the scene has a binding)
    assert bits_equal(got, oracle_canvas(oracle, sky, scn, rd, sd))


# ---- 9. partitions and groups --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_group_reproduces_the_single_handle(T, sky, world):
    scn = white_scene()
    single, textured, rd, _ = render_canvas(T, sky, scn, S.default_camera(), 0, textures=TEXTURES, bindings=white_bindings(TR.LINEAR))
    assert textured
    g = T.TracerGroup(W, H, n_devices=world, devices=[0] * world, rows_per_block=4)
    g.set_skybox(sky)
    g.options = rd
    g.scene_data = R.scene_data(len(scn[0]))
    g.set_textures(TEXTURES)
    g.set_material_textures(white_bindings(TR.LINEAR))
    g.update_scene(*scn)
    g.clear_canvas()
    g.render(1)
    got = g.read_canvas()
    g.close()
    assert bits_equal(got, single)


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_handles_reproduce_the_single_handle(T, sky, world):
    scn = white_scene()
    single, _, rd, _ = render_canvas(T, sky, scn, S.default_camera(), 0, textures=TEXTURES, bindings=white_bindings(TR.NEAREST))
    full = np.zeros_like(single)
    for rank in range(world):
        t = make(T, sky, scn, W, H, spp=4, time=4242)
        t.options = rd
        t.set_partition(rank, world, 4)
        t.set_textures(TEXTURES)
        t.set_material_textures(white_bindings(TR.NEAREST))
        t.clear_canvas()
        t.render(1)
        part = t.read_canvas()
        assert t.last_trace_textured()
        for r in range(t.owned_rows):
            full[T.global_row(H, rank, world, 4, r)] = part[r]
        t.close()
    assert bits_equal(full, single)


# ---- 11. the temporal history ------------------------------------------------------------------------------------------------
def test_each_setter_drops_the_history(T, sky):
    shapes, tris, mats, cam = guide_scene("mesh_flat")
    t = make(T, sky, (shapes, tris, mats), W, H, spp=2, cam=cam, denoise=dict(), temporal=dict())

    def frame():
        t.render(1)
        t.clear_canvas()  # the commit: the frame becomes the history
        return t.read_denoise_history()["valid"]

    assert frame()
    t.set_textures([TR.checker()])
    assert not t.read_denoise_history()["valid"]
    assert frame()
    t.set_material_textures(bind_all(len(mats), lambda i: 0))
    assert not t.read_denoise_history()["valid"]
    assert frame()
    t.set_triangle_uvs(np.zeros((len(tris), 3, 2), F))
    assert not t.read_denoise_history()["valid"]
    assert frame()
    t.close()


@pytest.mark.parametrize("limit,spp", [(32, 2), (5, 2)])
def test_still_camera_textured_bit_exact(T, sky, limit, spp):
    """tests/test_gpu_denoise_temporal.py's still-camera check on a textured scene: the temporal set-up and the committed
    history equal tests/temporal_ref.py bit for bit, the history's albedo guide being the texels'."""
    w, h = 80, 48
    tp = dict(history_limit=limit, normal_threshold=0.9, depth_threshold=0.05)
    shapes, tris, mats, textures, bindings = S.textured_sphere_scene()
    t = make(T, sky, (shapes, tris, mats), w, h, spp=spp, denoise=dict(iterations=0), temporal=tp)
    untex_albedo = None
    for textured in (False, True):
        if textured:
            t.set_textures(textures)
            t.set_material_textures(bindings)
            t.clear_canvas()
        hist = dict(valid=False)
        for f in range(4):
            t.options["time"] = 1000 + 17 * f
            argb = t.render(1).copy()
            assert t.last_trace_textured() == textured
            inp = t.read_denoise_inputs()
            want = temporal_ref.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, **tp)
            got = t.read_denoised()
            assert bits_equal(got[..., :3], want["c"]) and bits_equal(got[..., 3], want["V"]), (textured, f)
            assert np.array_equal(argb.reshape(h, w, 4), D.tonemap(want["c"])), (textured, f)
            if f == 0 and not textured:
                untex_albedo = inp["albedo_hits"].copy()
            if f == 0 and textured:
                assert not bits_equal(inp["albedo_hits"], untex_albedo)  # the guide sees texels
            t.clear_canvas()
            got_h = t.read_denoise_history()
            assert got_h["valid"]
            for k in ("colour", "count", "m1", "m2", "guide"):
                assert bits_equal(got_h[k], want["commit"][k]), (textured, f, k)
            hist = got_h
        assert hist["count"].max() == min(limit, 4 * spp)
    t.close()


# ---- 10. the denoiser keeps the pattern ------------------------------------------------------------------------------------
# Measured on an MI355X (160x90, 4 spp, default filter, tonemapped MSE against 4096 spp): see QUALITY_RATIO below.
QUALITY_RATIO = 0.6454  # measured: noisy MSE 1.967e-2, texel-guided 2.415e-3, colour-guided 3.742e-3; the threshold is halfway between it and 1 (0.8227)


def test_denoiser_keeps_the_pattern(T, sky):
    """Checker floor, gradient wall, striped sphere (scenes.textured_sphere_scene), 160x90, 4 spp, default filter, tonemapped
    MSE against a 4096-spp textured image. Texel-guided: the library's own filter result (the albedo guide is the texel at the
    first hit). Colour-guided: the same canvas, normals, depths and moments through tests/denoise_ref.py (the numpy filter the
    GPU filter is pinned to) with the albedo guide of an untextured run of the same rays, i.e. the material colours -- what
    the guide was before textures; no test-only switch in the library. The texel-guided error must be the lower one, by the
    threshold halfway between the measured ratio and 1."""
    w, h = 160, 90
    shapes, tris, mats, textures, bindings = S.textured_sphere_scene()

    def tracer(spp, time, textured=True):
        t = make(T, sky, (shapes, tris, mats), w, h, spp=spp, denoise={}, time=time)
        if textured:
            t.set_textures(textures)
            t.set_material_textures(bindings)
            t.clear_canvas()
        t.render(1)
        return t

    t = tracer(4096, 4242)
    ref = tone(t.read_canvas()[..., :3])
    t.close()
    t = tracer(4, 31)
    canvas, inp, den = t.read_canvas(), t.read_denoise_inputs(), t.read_denoised()[..., :3]
    t.close()
    t = tracer(4, 31, textured=False)
    colour_albedo = t.read_denoise_inputs()["albedo_hits"]
    t.close()
    F = 1  # default feature_samples
    ours = D.denoise(canvas, inp["normal_depth"], inp["albedo_hits"], inp["moments"], inp["T"], inp["P"], F, 1)[0][..., :3]
    np.testing.assert_allclose(den, ours, rtol=1e-4, atol=1e-6)  # the numpy filter is the GPU's
    forced = D.denoise(canvas, inp["normal_depth"], colour_albedo, inp["moments"], inp["T"], inp["P"], F, 1)[0][..., :3]
    mse_noisy = float(np.mean((tone(canvas[..., :3]) - ref) ** 2))
    mse_texel = float(np.mean((tone(den) - ref) ** 2))
    mse_colour = float(np.mean((tone(forced) - ref) ** 2))
    ratio = mse_texel / mse_colour
    print(f"textured quality: noisy MSE {mse_noisy:.4e}, texel-guided {mse_texel:.4e}, colour-guided {mse_colour:.4e}, ratio {ratio:.4f}")
    assert mse_texel < mse_colour
    assert QUALITY_RATIO is not None, "the ratio has not been measured yet"
    assert ratio <= (QUALITY_RATIO + 1.0) / 2.0, ratio


# ---- validation at the device ----------------------------------------------------------------------------------------------
def test_bad_bindings_fail_at_update_scene_and_render(T, sky):
    shapes, tris, mats, cam = guide_scene("mesh_flat")
    t = make(T, sky, (shapes, tris, mats), W, H, cam=cam)
    t.set_textures([TR.checker()])
    t.set_material_textures(bind_all(len(mats), lambda i: 1))  # only image 0 exists
    with pytest.raises(T.SrtError):
        t.render(1)
    with pytest.raises(T.SrtError):
        t.update_scene(shapes, tris, mats)
    t.set_material_textures(bind_all(len(mats), lambda i: 0))
    t.update_scene(shapes, tris, mats)
    t.set_triangle_uvs(np.zeros((len(tris) + 1, 3, 2), F))
    with pytest.raises(T.SrtError):
        t.update_scene(shapes, tris, mats)
    t.set_triangle_uvs(None)
    t.update_scene(shapes, tris, mats)
    t.render(1)
    assert t.last_trace_textured()
    t.set_material_textures(None)
    t.render(2)
    assert not t.last_trace_textured()
    t.close()


# ---- 12. srt_headless ------------------------------------------------------------------------------------------------------------
def test_headless_texture_equals_the_ctypes_route(T, tmp_path):
    """srt_headless --obj (with vt) --texture: the UVs it hands the library are the file's, the texels host/skybox.hpp's, and
    its bytes are those of the same calls through ctypes."""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    obj = tmp_path / "quad.obj"
    obj.write_text("v -1.5 -1.5 0\nv 1.5 -1.5 0\nv 1.5 1.5 0\nv -1.5 1.5 0\nvt 0 0\nvt 2 0.25\nvt 2.5 3\nvt -0.5 1\nvn 0 0 1\n"
                   "f 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\nf 2/2 3 4//1\n")
    img = (np.random.default_rng(9).integers(0, 256, (6, 5, 3))).astype(np.uint8)
    ppm = tmp_path / "tex.ppm"
    ppm.write_bytes(b"P6\n5 6\n255\n" + img.tobytes())
    pre = tmp_path / "h"
    w, h = 64, 48
    subprocess.run([str(exe), "--scene", "empty", "--obj", str(obj), "--width", str(w), "--height", str(h), "--spp", "4", "--texture", str(ppm),
                    "--texture-material", "0", "--texture-scale", "1.5", "--dump", str(pre)], check=True, timeout=120)
    rd = np.fromfile(f"{pre}.rd.bin", R.RENDER_DATA).reshape(())
    sd = np.fromfile(f"{pre}.sd.bin", R.SCENE_DATA).reshape(())
    shapes, tris, mats = np.fromfile(f"{pre}.shapes.bin", R.SHAPE), np.fromfile(f"{pre}.tris.bin", R.TRIANGLE), np.fromfile(f"{pre}.mats.bin", R.MATERIAL)
    sky_h = np.fromfile(f"{pre}.sky.bin", np.float32).reshape(1024, 2048, 4)
    texels = np.fromfile(f"{pre}.texture.bin", np.float32).reshape(6, 5, 4)
    uvs = np.fromfile(f"{pre}.uvs.bin", np.float32).reshape(-1, 3, 2)
    assert bits_equal(texels, S.skybox_from_rgb8(img))
    assert len(uvs) == len(tris) == 15 and not uvs[:12].any()  # the 12 box triangles have no UVs
    vt = np.array([[0, 0], [2, 0.25], [2.5, 3], [-0.5, 1]], F)
    assert np.array_equal(uvs[12], vt[[0, 1, 2]]) and np.array_equal(uvs[13], vt[[0, 2, 3]])
    assert np.array_equal(uvs[14], np.array([vt[1], [0, 0], [0, 0]], F))  # corners without vt: (0, 0)
    want = np.fromfile(f"{pre}.argb.bin", np.uint8)
    t = T.Tracer(w, h)
    t.set_skybox(sky_h)
    t.set_textures([texels])
    t.set_material_textures(bind_all(len(mats), lambda i: 0, filt=TR.LINEAR, scale=(1.5, 1.5)))
    t.set_triangle_uvs(uvs)
    t.scene_data = sd.copy()
    t.scene_data["num_shapes"] = 0  # as Tracer::update_scene before its first call
    t.clear_canvas()
    t.update_scene(shapes, tris, mats)
    t.options = rd.copy()
    out = t.render(1)
    assert t.last_trace_textured()
    assert np.array_equal(out, want)
    untextured = T.Tracer(w, h)
    untextured.set_skybox(sky_h)
    untextured.scene_data = t.scene_data.copy()
    untextured.update_scene(shapes, tris, mats)
    untextured.clear_canvas()
    untextured.options = rd.copy()
    assert not np.array_equal(untextured.render(1), want)  # the texture shows
    untextured.close()
    t.close()
