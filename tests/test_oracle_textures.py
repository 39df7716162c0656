"""CPU: what earns the textured form of the oracle (oracle/srt_oracle.c orc_*_textured; include/srt_abi.h "albedo textures")
its trust before tests/test_gpu_texture_paths.py holds the kernels' canvases to it. With nothing bound it is the untextured
oracle bit for bit (which tests/test_oracle_vs_ref.py pins to the reference); a texture of equal texels is a colour; at the
first hit it equals the independent numpy restatement (tests/texture_ref.py) on every first-hit case; its sampler equals
texture_ref.sample over hostile coordinates; two one-path cases have their answer written out here in float32; and every
scene the GPU tests use really looks textures up beyond the first hit (the coverage condition)."""
import numpy as np
import pytest

import golden_io
import texture_cases as TC
import texture_ref as TR
from conftest import bits_equal
from gpu_harness import SCENES, guide_scene
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
W, H = 37, 29
GOLDEN = golden_io.load_cases()


def frame_ids(w, h, ns):
    return np.repeat(np.arange(w * h), ns), np.tile(np.arange(ns), w * h)


# ---- nothing bound ---------------------------------------------------------------------------------------------------------------
def nothing_bound_tables(scn):
    """no table; images but every binding -1; a binding on a material no shape uses (appended) -> [(mats, table)]"""
    shapes, tris, mats = scn
    none = TC.bind_all(len(mats), lambda i: -1)
    more = R.concat(R.MATERIAL, mats, np.array([R.material(color=(0.3, 0.6, 0.9))], R.MATERIAL))
    unused = TC.bind_all(len(more), lambda i: 0 if i == len(more) - 1 else -1, filt=TR.LINEAR)
    images = [TR.checker(), TR.gradient()]
    return [(mats, None), (mats, TC.oracle_table(scn, images, none)), (more, TC.oracle_table((shapes, tris, more), images, unused))]


@pytest.mark.parametrize("name,accel", [s for s in SCENES if s[1] == 0])  # (the oracle has one traversal: accel is the kernels')
def test_nothing_bound_is_the_untextured_oracle(oracle, sky, name, accel):
    shapes, tris, mats, cam = guide_scene(name)
    rd, sd = R.render_data(W, H, 4, 10, camera_to_world=cam, time=4242), R.scene_data(len(shapes))
    want, wc = oracle.render(rd, sd, shapes, tris, mats, sky, counters=True)
    nd, ah = oracle.features(rd, sd, shapes, tris, mats, 3)
    ids, smp = frame_ids(W, H, 4)
    paths = oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, smp)
    for m, table in nothing_bound_tables((shapes, tris, mats)):
        got, gc = oracle.render_textured(rd, sd, shapes, tris, m, sky, table, counters=True)
        assert bits_equal(got, want) and gc == wc, name
        nd2, ah2 = oracle.features_textured(rd, sd, shapes, tris, m, table, 3)
        assert bits_equal(nd2, nd) and bits_equal(ah2, ah)
        L, looks = oracle.trace_paths_textured(rd, sd, shapes, tris, m, sky, table, ids, smp)
        assert bits_equal(L, paths) and not looks.any()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_committed_goldens_with_nothing_bound(oracle, sky, name):
    g = GOLDEN[name]
    scn = (g["shapes"], g["tris"], g["mats"])
    for m, table in nothing_bound_tables(scn):
        canvas = None
        for tm in g["frames"]:
            rd = g["rd"].copy()
            rd["time"] = np.uint32(tm)
            canvas = oracle.render_textured(rd, g["sd"], g["shapes"], g["tris"], m, sky, table, canvas=canvas)
        assert bits_equal(canvas, g["canvas"]), name


# ---- constant texture = colour -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 4])
@pytest.mark.parametrize("name,accel", [s for s in SCENES if s[1] == 0 and s[0] != "empty"])
def test_constant_texture_is_the_colour(oracle, sky, name, accel, side):
    shapes, tris, mats, cam = guide_scene(name)
    rd, sd = R.render_data(W, H, 4, 10, camera_to_world=cam, time=4242), R.scene_data(len(shapes))
    table = TC.oracle_table((shapes, tris, mats), TC.constant_textures(mats, side), TC.bind_all(len(mats), lambda i: i, scale=(3.0, -2.5)))
    want = oracle.render(rd, sd, shapes, tris, mats, sky)
    got = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table)
    assert bits_equal(got, want), (name, side)
    _, looks = oracle.trace_paths_textured(rd, sd, shapes, tris, mats, sky, table, *frame_ids(W, H, 4))
    assert looks.sum() > 0  # the texels were really read
    # ... and the texel REPLACES the colour wherever the colour is used (mix and the refracted mask): the same textures over
    # materials painted another colour still give the untextured oracle's canvas of the original colours
    grey = mats.copy()
    grey["color"][:, :3] = F(0.5)
    got = oracle.render_textured(rd, sd, shapes, tris, grey, sky, table)
    assert bits_equal(got, want), (name, side, "repainted")
    assert name == "empty" or not bits_equal(oracle.render(rd, sd, shapes, tris, grey, sky), want)


def test_back_face_sphere_uv_takes_the_unflipped_normal(oracle, sky):
    """The camera inside a textured sphere: every first hit is a back face, and the UV is made from (X - centre) / radius,
    not from the shading normal (which is flipped there)."""
    scn = TC.white_scene()
    shapes, tris, mats = scn
    bindings = TC.bind_all(5, lambda i: 1, filt=TR.LINEAR, scale=(2.0, 1.0))
    cam = R.camera_matrix((1.9, 0.7, -1.8), 0.4, 0.1)  # inside sphere 2 (centre (1.7, 0.8, -2.0), radius 1.3)
    rd, sd = R.render_data(W, H, 2, 2, camera_to_world=cam, time=5), R.scene_data(len(shapes))
    ph = oracle.primary_hits(rd, sd, shapes, tris, mats, np.arange(W * H), np.zeros(W * H, np.int32))
    assert (ph["material"] == 2).all()
    want = np.zeros((W * H, 3), F)
    for k in range(2):
        tex, _ = TC.first_hit_texels(oracle, rd, sd, scn, bindings, np.arange(W * H), np.full(W * H, k))
        want = (want + tex).astype(F)
    _, ah = oracle.features_textured(rd, sd, shapes, tris, mats, TC.oracle_table(scn, TC.TEXTURES, bindings), 2)
    assert bits_equal(ah[..., :3].reshape(-1, 3), want)


# ---- agreement with the numpy restatement at the first hit ---------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [TR.LINEAR, TR.NEAREST])
@pytest.mark.parametrize("kind,accel,with_uvs", TC.FIRST_HIT_CASES)
def test_first_hit_agrees_with_texture_ref(oracle, sky, kind, accel, with_uvs, filt):
    """orc_features_textured = the sum of texture_ref texels at orc_primary_hits; the two-bounce white canvas of
    orc_render_textured = texel * L_white -- on the cases and by the expressions of tests/test_gpu_texture.py."""
    scn, bindings, uvs = TC.first_hit_case(kind, filt, with_uvs)
    shapes, tris, mats = scn
    table = TC.oracle_table(scn, TC.TEXTURES, bindings, uvs)
    ns, fs = 4, 3
    rd, sd = R.render_data(W, H, ns, 2, camera_to_world=S.default_camera(), time=99), R.scene_data(len(shapes))
    want = np.zeros((W * H, 3), F)
    for k in range(fs):
        tex, _ = TC.first_hit_texels(oracle, rd, sd, scn, bindings, np.arange(W * H), np.full(W * H, k), uvs)
        want = (want + tex).astype(F)
    nd, ah = oracle.features_textured(rd, sd, shapes, tris, mats, table, fs)
    nd0, ah0 = oracle.features(rd, sd, shapes, tris, mats, fs)
    assert bits_equal(nd, nd0) and bits_equal(ah[..., 3], ah0[..., 3])
    assert not bits_equal(ah[..., :3], ah0[..., :3])
    assert bits_equal(ah[..., :3].reshape(-1, 3), want), (kind, with_uvs, filt)
    ids, smp = frame_ids(W, H, ns)
    L = oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, smp).astype(F)
    tex, hit = TC.first_hit_texels(oracle, rd, sd, scn, bindings, ids, smp, uvs)
    rad = np.where(hit[:, None], (tex * L).astype(F), L).reshape(W * H, ns, 3)
    canvas = np.zeros((W * H, 3), F)
    for k in range(ns):
        canvas = (canvas + rad[:, k]).astype(F)
    canvas = (canvas / F(ns)).astype(F)
    got = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table)
    assert bits_equal(got[..., :3].reshape(-1, 3), canvas), (kind, with_uvs, filt)
    Lt, looks = oracle.trace_paths_textured(rd, sd, shapes, tris, mats, sky, table, ids, smp)
    assert bits_equal(Lt, rad.reshape(-1, 3)) and not looks[:, 1].any() and np.array_equal(looks[:, 0] > 0, hit)


# ---- the sampler directly -------------------------------------------------------------------------------------------------------------
def hostile_coordinates(rng, w, h, scale, n=100_000):
    """(u, v) before the scale: uniform in +-3 (negative values), exact texel integers and half-integers, the floats just
    below and above +-2^30 after the scale and the image size, +-0, +-inf, NaN"""
    u, v = rng.uniform(-3, 3, n).astype(F), rng.uniform(-3, 3, n).astype(F)
    k = rng.integers(-4 * w, 4 * w, n // 4)
    u[: n // 4] = (k.astype(F) * F(0.5)) / F(w) / F(scale[0])  # integers and half-integers of the texel grid (about: the divisions round)
    k = rng.integers(-4 * h, 4 * h, n // 4)
    v[n // 8: n // 8 + n // 4] = (k.astype(F) * F(0.5)) / F(h) / F(scale[1])
    edge = []
    for size, s in ((w, scale[0]), (h, scale[1])):
        x = F(2.0 ** 30) / F(size) / F(abs(s))
        e = [x]
        for _ in range(3):
            e = [np.nextafter(e[0], F(0))] + e + [np.nextafter(e[-1], F(np.inf))]
        edge.append(np.array(e + [-t for t in e] + [0.0, -0.0, np.inf, -np.inf, np.nan, 0.5, -0.5, 1.0], F))
    eu, ev = np.meshgrid(edge[0], edge[1])
    m = eu.size
    u[-m:], v[-m:] = eu.reshape(-1), ev.reshape(-1)
    u[-2 * m:-m], v[-2 * m:-m] = eu.reshape(-1), rng.uniform(-3, 3, m).astype(F)  # one hostile coordinate, one ordinary
    u[-3 * m:-2 * m], v[-3 * m:-2 * m] = rng.uniform(-3, 3, m).astype(F), ev.reshape(-1)
    return u, v


@pytest.mark.parametrize("filt", [TR.LINEAR, TR.NEAREST])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (16, 8)])
def test_sampler_equals_texture_ref(oracle, filt, w, h):
    rng = np.random.default_rng(100 * w + h)
    image = np.ones((h, w, 4), F)
    image[..., :3] = rng.uniform(0, 1, (h, w, 3)).astype(F)
    for scale in ((1.0, 1.0), (-2.5, 0.37), (1e30, -3e38)):
        u, v = hostile_coordinates(rng, w, h, scale)
        got = oracle.sample_texture(image, filt, u, v, *scale)
        want = TR.sample(image, filt, u, v, *scale)
        assert bits_equal(got, want), (w, h, filt, scale, int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))


# ---- hand-computed deep paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specular", [0.0, 1.0])
def test_mirror_then_plane_then_sky_by_hand(oracle, sky, specular):
    """One camera ray: a perfect mirror sphere (metallic 1, smoothness 1, textured), then a textured diffuse plane, then the
    sky. Both textures are 1x1 and sampled NEAREST, so the texels are the constants below whatever the UVs: the answer needs neither restatement
    of the UV rules. The sky radiance of that very path is the UNTEXTURED oracle's on white materials (every mask factor is
    exactly 1 there, and a lookup draws no random number). mask = ((1 * f) * texel_plane) with f = mix(texel_sphere, 1,
    is_specular) = texel_sphere, or texel_sphere + (1 - texel_sphere) * 1 for specular = 1; radiance = mask * sky."""
    # mix(t, 1, 1) = fma(1 - t, 1, t) is 1.0f for every t in [0, 1] (the rounding error of 1 - t is at most half an ulp of 1);
    # it is not where 1 - t rounds by more: t = 2^24 + 2 gives 2, t = 5e8 gives 0. Such texels are finite and not negative.
    ts = np.array([0.3, 0.61, 0.0123] if specular == 0.0 else [16777218.0, 0.61, 5e8], F)
    tp = np.array([0.77, 0.2, 0.55], F)
    mats = np.array([R.material(color=(1, 1, 1), metallic=1.0, smoothness=1.0, specular=specular), R.material(color=(1, 1, 1))], R.MATERIAL)
    shapes = np.array([R.sphere(0, (0.0, 0.5, 0.0), 1.0), R.plane(1, (0.0, -0.5, 0.0), (0.0, 1.0, 0.0))], R.SHAPE)
    tris = np.zeros(0, R.TRIANGLE)
    images = [np.append(ts, F(1)).reshape(1, 1, 4), np.append(tp, F(1)).reshape(1, 1, 4)]
    bindings = np.array([R.material_texture(0, TR.NEAREST, 2.5, -1.5), R.material_texture(1, TR.NEAREST, 0.3, 4.0)], R.MATERIAL_TEXTURE)
    table = TC.oracle_table((shapes, tris, mats), images, bindings)
    rd, sd = R.render_data(W, H, 1, 3, camera_to_world=S.default_camera(), time=7), R.scene_data(2)
    ids, smp = frame_ids(W, H, 1)
    white = oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, smp)
    got, looks = oracle.trace_paths_textured(rd, sd, shapes, tris, mats, sky, table, ids, smp)
    first = oracle.primary_hits(rd, sd, shapes, tris, mats, ids, smp)["material"]
    # sphere, then something textured (only the plane: a reflection off a sphere leaves it), then the sky (radiance > 0: a third hit adds 0)
    sel = np.flatnonzero((first == 0) & (looks[:, 0] == 1) & (looks[:, 1] == 1) & (white > 0).all(axis=1))
    assert len(sel) >= 10
    one = F(1)
    f = ts if specular == 0.0 else (ts + (one - ts) * one).astype(F)
    if specular == 1.0:
        assert np.array_equal(f, np.array([2.0, 1.0, 0.0], F))  # the texel's bits matter where a colour "is ignored"
    for k in sel[:10]:
        sky_k = white[k].astype(F)
        mask = ((one * f).astype(F) * tp).astype(F)
        want = (mask * sky_k).astype(F)
        assert bits_equal(got[k], want), (k, got[k], want)


# ---- the coverage condition of tests/test_gpu_texture_paths.py ---------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [TR.LINEAR, TR.NEAREST])
@pytest.mark.parametrize("name,with_uvs,w,h", TC.GPU_VIEWS)
def test_path_cases_look_textures_up_beyond_the_first_hit(oracle, sky, name, with_uvs, w, h, filt):
    """Every (case, frame) tests/test_gpu_texture_paths.py renders: at least one path in five reads a texel at its second or a
    later hit, and the canvas differs in more than a tenth of its pixels from the canvas with only the first hit's texel
    applied. Where the floor has its specular coat, at least ten paths make a specular bounce on a texel whose
    mix(texel, 1, 1) is not 1.0f (texture_cases.coat_texture): replacing that mix by 1 changes the canvas."""
    case = TC.path_case(name, filt, with_uvs, w=w, h=h)
    rd, sd = TC.case_render_data(case)
    assert (case["w"], case["h"]) == (w, h)
    shapes, tris, mats = case["scn"]
    table = TC.oracle_table(case["scn"], case["images"], case["bindings"], case["uvs"])
    ids, smp = frame_ids(w, h, case["spp"])
    L, looks = oracle.trace_paths_textured(rd, sd, shapes, tris, mats, sky, table, ids, smp)
    assert (looks[:, 1] > 0).mean() >= 0.2, (name, (looks[:, 1] > 0).mean())
    if name in ("material", "material_pad"):
        assert (looks[:, 2] > 0).sum() >= 10, (name, (looks[:, 2] > 0).sum())
    full = TC.oracle_path_canvas(oracle, sky, case)
    first_only = TC.oracle_path_canvas(oracle, sky, case, first_hit_only=True)
    differ = (full.view(np.uint32) != first_only.view(np.uint32)).any(axis=-1).mean()
    assert differ > 0.1, (name, differ)
    assert np.isfinite(full).all()
    # the canvas is the per-path radiances summed in sample order
    rad = L.reshape(w * h, case["spp"], 3)
    acc = np.zeros((w * h, 3), F)
    for k in range(case["spp"]):
        acc = (acc + rad[:, k]).astype(F)
    assert bits_equal(full[..., :3].reshape(-1, 3), (acc / F(case["spp"])).astype(F))
