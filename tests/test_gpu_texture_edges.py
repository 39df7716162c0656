"""GPU (MI355X): the albedo-texture sampler of the textured kernels (csrc/device_shading.h sample_texture under texture_albedo)
at coordinates the test chooses -- the images, pairs and scenes of tests/texture_edge_cases.py, whose claims (the crafted route
hands the sampler u = v = 1.0f, coverage of every column, row, wrap and side of the guard, mutants of the rule)
tests/test_texture_edge_cases.py asserts on the CPU. One 8 x 4 frame of one sample per coordinate pair, every pixel the same ray:
the denoiser's albedo guide (the feature kernels' copy of the sampler) is the restatement's texel (tests/texture_ref.py) in every
pixel, the two-bounce canvas (the trace kernels' copy) is the textured C oracle's. One handle serves a scene and an image set;
between pairs only the bindings change. Every comparison is exact: bits, NaN equal to NaN. No expected value comes from a device."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as FS
import texture_edge_cases as EC
import texture_ref as TR
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
F = np.float32
IMAGES = EC.images()
DEEP = EC.deep_set(IMAGES)
W, H = EC.FRAME
N = W * H
GENERAL = 0  # device_types.h SRT_SCENE_CLASS_LIST: textured dispatches run the general kernels, whose instantiation the scene decides
ROUTE_IMAGES = ["3x2", "7x1", "4099x3"]


def tracer(T, sky, scn, cam, fov, w, h, accel, image_set, uvs=None):
    shapes, tris, mats = scn
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    t.options = EC.render_data(cam, fov, w, h)
    t.scene_data = EC.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.set_denoise(feature_samples=1, iterations=0)
    t.set_textures(image_set)
    if uvs is not None:
        t.set_triangle_uvs(uvs)
    return t


def frame(t, bindings):
    """one cleared frame under `bindings` -> guide (h * w, 4), canvas (h * w, 4)"""
    t.set_material_textures(bindings)
    t.clear_canvas()
    t.render(1)
    assert t.last_trace_textured()
    return t.read_denoise_inputs()["albedo_hits"].reshape(-1, 4), t.read_canvas().reshape(-1, 4)


def crafted_frames(t, oracle, sky, scn, image_set, index, filt, ps, what):
    """Every pair of ps on a crafted handle: guide = the restatement's texel in every pixel (0 + texel: the guide is a sum), one hit
    per pixel; canvas = the textured oracle's. -> [(guide, canvas)]

    One kind of texel has another expected canvas, and only the specials image holds it: an INFINITE channel. The header expects
    texels finite and not negative, and DESIGN.md 13 ("SRT_MF_PLAIN_COLORS and texels") records what happens outside that: on
    materials without a specular coat the kernels multiply the mask by the texel where the oracle takes mix(texel, 1, 0) =
    fma(1 - texel, 0, texel), which is the texel for every finite one and NaN for an infinite one. For such a channel the expected
    value is the product itself, 0 + texel * L with L the untextured oracle's radiance of the same path on the white scene (the
    identity tests/test_texture_edge_cases.py holds the oracle to for every finite texel). The guide is the sampler's output
    whatever the texel."""
    shapes, tris, mats = scn
    rd, sd = t.options, t.scene_data
    ids = np.arange(N, dtype=np.int32)
    L = oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, np.zeros_like(ids)).astype(F)
    table = EC.oracle_table(scn, image_set, EC.binding(len(mats), index, filt, 1.0, 1.0))
    want = TR.sample(image_set[index], filt, *EC.pair_scales(ps))
    out = []
    for p, tex in zip(ps, want):
        guide, canvas = frame(t, EC.binding(len(mats), index, filt, p["su"], p["sv"]))
        assert bits_equal(guide[:, :3], np.tile(F(0) + tex, (N, 1))), (what, p["name"], guide[0], tex)
        assert guide[:, 3].sum() == N, (what, p["name"])
        table.bindings[0]["scale_u"], table.bindings[0]["scale_v"] = p["su"], p["sv"]
        with np.errstate(all="ignore"):
            oc = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table).reshape(-1, 4)
            if np.isinf(tex).any():
                oc[:, :3] = np.where(np.isinf(tex)[None, :], F(0) + (tex[None, :] * L).astype(F), oc[:, :3])
        assert bits_equal(canvas, oc), (what, p["name"], FS.differing_pixels(canvas, oc))
        out.append((guide, canvas))
    return out


def check_route(t, scn, route):
    """Which instantiation ran. A textured dispatch reports class 0 and plane form 0 whatever the scene (the scene classes and their
    axis twins are built for untextured dispatches alone); what tells the general kernels apart is what the launcher picks them
    by: models or none, a hierarchy or the array scan, and whether the scene records fit the LDS copy."""
    shapes, _, mats = scn
    assert (t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured()) == (GENERAL, 0, True), route
    models = int((shapes["type"] == 2).sum())
    assert (models > 0) == (route in ("scan", "bvh"))
    assert (t.acceleration_info()["nodes"] > 0) == (route == "bvh"), (route, t.acceleration_info())
    if not models:
        assert (FS.scene_lds_bytes(len(shapes), len(mats)) == 0) == (route == "pad")


# ---- the z plane: every pair of every image ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", list(IMAGES))
def test_z_plane_every_pair(name, filt, T, sky, oracle):
    scn, cam, accel = EC.crafted_scene("z")
    t = tracer(T, sky, scn, cam, 0.0, W, H, accel, [IMAGES[name]])
    try:
        ps = EC.pairs(IMAGES[name], filt)
        crafted_frames(t, oracle, sky, scn, [IMAGES[name]], 0, filt, ps, (name, filt))
        check_route(t, scn, "alone")
    finally:
        t.close()


# ---- the other instantiations and orientations: integers, half-integers, the guard -------------------------------------------------------
@pytest.mark.parametrize("route", EC.ROUTES)
@pytest.mark.parametrize("axis", list(EC.CRAFTED))
def test_routes_and_orientations(axis, route, T, sky, oracle):
    """Sphere / plane kernel, model scan, BVH walk and records outside the LDS copy, for a plane along each axis: the subset on three
    images (one handle each), both filters. The guide is the restatement's on every route, so the routes agree bit for bit; the
    canvas is the oracle's of that route's scene."""
    scn, cam, accel = EC.crafted_scene(axis, route)
    for name in ROUTE_IMAGES:
        t = tracer(T, sky, scn, cam, 0.0, W, H, accel, [IMAGES[name]])
        try:
            for filt in EC.FILTERS:
                ps = EC.pairs(IMAGES[name], filt, subset=True)
                crafted_frames(t, oracle, sky, scn, [IMAGES[name]], 0, filt, ps, (axis, route, name, filt))
            check_route(t, scn, route)
        finally:
            t.close()


# ---- UVs as they come: tilted plane, sphere, mesh -------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name,accel", [("tilted", 0), ("sphere", 0), ("sphere_tall", 0), ("mesh", 0), ("mesh", 1)])
def test_compared_scenes(name, accel, filt, T, sky, oracle):
    """Every camera of the case (the fixed ones at the sphere's poles and seam on 8 x 4, the moving ones on 37 x 29 and 33 x 7): the
    guide is texture_ref.sample at texture_ref's UV of the oracle's primary hit (albedo 1 where nothing is hit) and the oracle's
    own guide; the canvas is the oracle's."""
    case = EC.compared_cases(IMAGES)[name]
    shapes, tris, mats = case["scn"]
    uvs = case["uvs"](filt) if case["uvs"] else None
    b = EC.binding(1, 0, filt, *case["scale"])
    table = EC.oracle_table(case["scn"], [case["image"]], b, uvs)
    handles = {}
    try:
        for cam, fov, w, h in case["cams"]:
            if (w, h) not in handles:
                handles[w, h] = tracer(T, sky, case["scn"], cam, fov, w, h, accel, [case["image"]], uvs)
            t = handles[w, h]
            t.options = EC.render_data(cam, fov, w, h)
            guide, canvas = frame(t, b)
            rd, sd = t.options, t.scene_data
            u, v, hit, _ = EC.hit_uvs(oracle, rd, sd, case["scn"], uvs)
            want = np.where(hit[:, None], TR.sample(case["image"], filt, u, v, *case["scale"]), F(1))
            assert bits_equal(guide[:, :3], want), (name, accel, filt, w, h, FS.differing_pixels(guide[:, :3], want))
            assert np.array_equal(guide[:, 3] == 1, hit)
            _, ah = oracle.features_textured(rd, sd, shapes, tris, mats, table, 1)
            assert bits_equal(guide, ah.reshape(-1, 4))
            with np.errstate(all="ignore"):
                oc = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table).reshape(-1, 4)
            assert bits_equal(canvas, oc), (name, accel, filt, w, h, FS.differing_pixels(canvas, oc))
            assert (t.acceleration_info()["nodes"] > 0) == (accel == 1)
    finally:
        for t in handles.values():
            t.close()


# ---- an image behind 63 others ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
def test_deep_set(filt, T, sky, oracle):
    """The image under test bound as image 63 of 64 (its offset is 35,861 texels): the bits of the same image uploaded alone, which
    are the restatement's and the oracle's. Then set_textures on the live handle, deep set -> one image -> deep set: the same bits
    each time."""
    image = IMAGES[EC.DEEP_IMAGE]
    last = EC.MAX_TEXTURES - 1
    scn, cam, accel = EC.crafted_scene("z")
    ps = EC.pairs(image, filt, subset=True)
    t = tracer(T, sky, scn, cam, 0.0, W, H, accel, DEEP)
    alone = tracer(T, sky, scn, cam, 0.0, W, H, accel, [image])
    try:
        deep = crafted_frames(t, oracle, sky, scn, DEEP, last, filt, ps, ("deep", filt))
        single = crafted_frames(alone, oracle, sky, scn, [image], 0, filt, ps, ("alone", filt))
        for p, d, s in zip(ps, deep, single):
            assert bits_equal(d[0], s[0]) and bits_equal(d[1], s[1]), p["name"]
        for image_set, index in (([image], 0), (DEEP, last), ([image], 0)):
            t.set_textures(image_set)
            again = crafted_frames(t, oracle, sky, scn, image_set, index, filt, ps[::3], ("live", len(image_set), filt))
            for d, a in zip(deep[::3], again):
                assert bits_equal(d[0], a[0]) and bits_equal(d[1], a[1])
    finally:
        t.close()
        alone.close()


# ---- groups and partitions -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_frames(T, sky, oracle):
    """(filter) -> the single handle's checked (guide, canvas) per pair of the 3x2 image's subset on the z plane: computed once"""
    scn, cam, accel = EC.crafted_scene("z")
    t = tracer(T, sky, scn, cam, 0.0, W, H, accel, [IMAGES["3x2"]])
    try:
        return {filt: crafted_frames(t, oracle, sky, scn, [IMAGES["3x2"]], 0, filt, EC.pairs(IMAGES["3x2"], filt, subset=True), ("single", filt))
                for filt in EC.FILTERS}
    finally:
        t.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_reproduces_the_single_handle(world, T, sky, single_frames):
    scn, cam, _ = EC.crafted_scene("z")
    g = T.TracerGroup(W, H, n_devices=world, devices=[0] * world, rows_per_block=1)
    try:
        g.set_skybox(sky)
        g.options = EC.render_data(cam, 0.0, W, H)
        g.scene_data = EC.scene_data(1)
        g.set_textures([IMAGES["3x2"]])
        g.update_scene(*scn)
        for filt in EC.FILTERS:
            for p, (_, canvas) in zip(EC.pairs(IMAGES["3x2"], filt, subset=True), single_frames[filt]):
                g.set_material_textures(EC.binding(1, 0, filt, p["su"], p["sv"]))
                g.clear_canvas()
                g.render(1)
                assert bits_equal(g.read_canvas().reshape(-1, 4), canvas), (world, filt, p["name"])
        for i in range(world):
            member, out = C.c_void_p(g.lib.srt_group_tracer(g._g, i)), C.c_int(-1)
            assert g.lib.srt_last_trace_textured(member, C.byref(out)) == 0 and out.value == 1, i
    finally:
        g.close()


def test_partition_of_three_reproduces_the_single_handle(T, sky, single_frames):
    """ranks 0..2 of 3 in blocks of one row: each rank's packed rows are the whole frame's"""
    scn, cam, accel = EC.crafted_scene("z")
    for rank in range(3):
        t = tracer(T, sky, scn, cam, 0.0, W, H, accel, [IMAGES["3x2"]])
        try:
            t.set_denoise(False)
            t.set_partition(rank, 3, 1)
            assert t.owned_rows > 0
            for filt in EC.FILTERS:
                for p, (_, canvas) in zip(EC.pairs(IMAGES["3x2"], filt, subset=True), single_frames[filt]):
                    t.set_material_textures(EC.binding(1, 0, filt, p["su"], p["sv"]))
                    t.clear_canvas()
                    t.render(1)
                    assert t.last_trace_textured()
                    part, whole = t.read_canvas(), canvas.reshape(H, W, 4)
                    for r in range(t.owned_rows):
                        assert bits_equal(part[r], whole[T.global_row(H, rank, 3, 1, r)]), (rank, filt, p["name"], r)
        finally:
            t.close()
