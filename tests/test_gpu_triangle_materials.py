"""GPU: per-triangle materials (srt_set_triangle_materials; include/srt_abi.h "per-triangle materials"). Every canvas here is
the CPU oracle's canvas of the SPLIT scene -- one model shape per run of triangles of one material,
tests/triangle_material_cases.py -- bit for bit, at ten bounces, so a wrong material at ANY hit of a path changes bits: a hit
record out of the wave's queue, out of a suspended scan or the ray pool, or the BVH's leaf reference. The shapes are the
texture path tests' own (tests/test_gpu_texture_paths.py); every (case, assignment, frame) rendered against the oracle is
listed in GPU_VIEWS there, and tests/test_triangle_materials_host.py asserts on each that the table changes at least a fifth
of the oracle's pixels."""
import numpy as np
import pytest

import motion_ref
import texture_cases as TC
import triangle_material_cases as M
from conftest import bits_equal
from gpu_harness import T, make  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu
SRT_ERR_INVALID = 1


def bind(t, case, tm="case"):
    t.set_textures(case["images"])
    t.set_material_textures(case["bindings"])
    t.set_triangle_uvs(case["uvs"])
    t.set_triangle_materials(case["tm"] if isinstance(tm, str) else tm)


def tracer(T, sky, case, accel=0, denoise=None, tm="case", **kw):
    t = make(T, sky, case["scn"], case["w"], case["h"], spp=case["spp"], accel=accel, time=case["time"], cam=case["cam"], denoise=denoise, **kw)
    t.options["num_bounces"] = case["bounces"]
    bind(t, case, tm)
    t.clear_canvas()
    return t


def differing(got, want):
    return f"{int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


def check(T, sky, oracle, case, accel, what=None):
    t = tracer(T, sky, case, accel)
    t.render(1)
    got, rd, sd = t.read_canvas(), t.options.copy(), t.scene_data.copy()
    assert t.last_trace_textured() == 1
    t.close()
    want = M.oracle_canvas(oracle, sky, case, rd, sd)
    assert bits_equal(got, want), (what, accel, differing(got, want))


# ---- canvas equals split oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", TC.FRAMES)
@pytest.mark.parametrize("textured", [True, False])
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("assignment", ["per_face", "interleaved"])
def test_mesh_equals_split_oracle(T, sky, oracle, assignment, accel, textured, w, h):
    """Diffuse, mirror, glass and specular-coat triangles inside one box, two instances over one triangle range; with textures
    and UVs bound, and with nothing bound at all: the table alone then reaches the textured kernels."""
    check(T, sky, oracle, M.tm_case("mesh", assignment, textured, w, h), accel, what=(assignment, textured, w, h))


@pytest.mark.parametrize("textured", [True, False])
@pytest.mark.parametrize("accel", [0, 1])
def test_materials_in_global_memory(T, sky, oracle, accel, textured):
    """80 more materials take the scene records out of LDS; the table points at materials 40..43"""
    case = M.tm_case("mesh_pad", "per_face", textured)
    assert case["tm"].max() > 7
    check(T, sky, oracle, case, accel, what=("mesh_pad", textured))


@pytest.mark.parametrize("accel", [0, 1])
def test_big_models(T, sky, oracle, accel):
    """Models of 128 and more triangles, every run of length 1: the array scan suspends their rays (the hit records come from
    the scan queue), the BVH hands back a leaf-block reference; with the triangle counters and without. tri_tests is not
    compared: the split scene's box tests see a smaller tmin."""
    case = M.tm_case("big", "interleaved", True, 64, 40)
    shapes, tris, mats = case["scn"]
    t = tracer(T, sky, case, accel)
    want, oc = M.oracle_canvas(oracle, sky, case, t.options.copy(), t.scene_data.copy(), counters=True)
    for count in (True, False):
        t.count_triangles(count)
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        got, c = t.read_canvas(), t.counters()
        assert t.last_trace_textured() == 1
        assert bits_equal(got, want), (accel, count, differing(got, want))
        for k in ("paths", "rays", "sky"):
            assert c[k] == oc[k], (k, c[k], oc[k])
        assert c["watchdog"] == 0
    if accel == 0:
        assert t.debug_counters()["scans"] > 0
    t.close()


# ---- tables that bind nothing, and a single entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_table_that_binds_nothing(T, sky, accel):
    case = M.tm_case("mesh", "all_minus_one", textured=False)
    t = tracer(T, sky, case, accel, tm=None)
    canvases = []
    for tm in ("never set", None, case["tm"]):
        if not isinstance(tm, str):
            t.set_triangle_materials(tm)
        t.clear_canvas()
        t.render(1)
        assert t.last_trace_textured() == 0
        canvases.append(t.read_canvas())
    t.close()
    assert bits_equal(canvases[1], canvases[0]) and bits_equal(canvases[2], canvases[0])


@pytest.mark.parametrize("textured", [True, False])
@pytest.mark.parametrize("accel", [0, 1])
def test_single_entry(T, sky, oracle, accel, textured):
    case = M.tm_case("mesh", "single", textured)
    assert int((case["tm"] >= 0).sum()) == 1
    check(T, sky, oracle, case, accel, what=("single", textured))


# ---- routes --------------------------------------------------------------------------------------------------------------------------
ROUTE_ACCEL = [0, 1]


@pytest.fixture(scope="module")
def route_case():
    return M.tm_case("mesh", "per_face", textured=False)


@pytest.fixture(scope="module")
def route_want(oracle, sky, route_case):
    return M.oracle_canvas(oracle, sky, route_case)


@pytest.mark.parametrize("accel", ROUTE_ACCEL)
def test_sample_batches(T, sky, route_case, route_want, accel):
    """two radiance buffers of one sample each: the four samples run as four launches that overlap on two streams"""
    case = route_case
    t = tracer(T, sky, case, accel)
    t.set_radiance_budget(case["w"] * case["h"] * 12 * 2)
    t.render(1)
    got = t.read_canvas()
    assert t.last_trace_launches() == (4, True) and t.last_trace_textured() == 1
    t.close()
    assert bits_equal(got, route_want), differing(got, route_want)


@pytest.mark.parametrize("accel", ROUTE_ACCEL)
def test_row_partition(T, sky, route_case, route_want, accel):
    case, world = route_case, 3
    full = np.zeros_like(route_want)
    for rank in range(world):
        t = tracer(T, sky, case, accel)
        t.set_partition(rank, world, 3)
        t.clear_canvas()
        t.render(1)
        part = t.read_canvas()
        assert t.last_trace_textured() == 1
        for r in range(t.owned_rows):
            full[T.global_row(case["h"], rank, world, 3, r)] = part[r]
        t.close()
    assert bits_equal(full, route_want), differing(full, route_want)


@pytest.mark.parametrize("accel", ROUTE_ACCEL)
def test_device_group(T, sky, route_case, route_want, accel):
    case = route_case
    rd, _ = TC.case_render_data(case)
    g = T.TracerGroup(case["w"], case["h"], n_devices=3, devices=[0] * 3, rows_per_block=3)
    g.set_skybox(sky)
    g.set_acceleration(accel)
    g.options = rd
    g.scene_data = R.scene_data(len(case["scn"][0]))
    bind(g, case)  # srt_group_set_triangle_materials: every member
    g.update_scene(*case["scn"])
    g.clear_canvas()
    g.render(1)
    got = g.read_canvas()
    g.close()
    assert bits_equal(got, route_want), differing(got, route_want)


# ---- the feature pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,assignment,textured,accel", [("mesh", "per_face", True, 0), ("mesh", "interleaved", False, 1), ("big", "interleaved", True, 0),
                                                            ("big", "interleaved", True, 1)])
def test_albedo_guide(T, sky, oracle, name, assignment, textured, accel):
    """feature_samples = spp: the albedo guide reads the material the trace kernel shades with; with object motion on, the
    shape ids are the unsplit scene's shape indices"""
    case = M.tm_case(name, assignment, textured, *((64, 40) if name == "big" else (37, 29)))
    shapes, tris, mats = case["scn"]
    t = tracer(T, sky, case, accel, denoise=dict(feature_samples=case["spp"], iterations=0), temporal={}, motion=True)
    t.render(1)
    inp, rd, sd = t.read_denoise_inputs(), t.options.copy(), t.scene_data.copy()
    ids = t.read_denoise_shape_ids()[0]
    assert t.last_trace_textured() == 1
    t.close()
    nd, ah = M.oracle_features(oracle, case, rd, sd, case["spp"])
    assert bits_equal(inp["normal_depth"], nd)
    assert bits_equal(inp["albedo_hits"], ah), (name, assignment, accel, differing(inp["albedo_hits"], ah))
    # the first hit of feature sample 0, a material per shape of the UNSPLIT scene naming the shape (tests/test_gpu_denoise_motion.py)
    own = np.frombuffer(bytearray(shapes.tobytes()), shapes.dtype)
    own["material"] = np.where(own["material"] >= 0, np.arange(len(own)), -1)
    n = case["w"] * case["h"]
    hit = oracle.primary_hits(rd, sd, own, tris, np.resize(mats, max(len(own), len(mats))), np.arange(n), np.zeros(n, np.int32))
    want_ids = np.where(hit["material"] >= 0, hit["material"], motion_ref.NO_SHAPE).astype(np.uint32).reshape(case["h"], case["w"])
    assert np.array_equal(ids, want_ids)


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_bad_tables_fail_at_update_scene_and_dispatch(T, sky):
    case = M.tm_case("mesh", "per_face", textured=False)
    shapes, tris, mats = case["scn"]
    t = tracer(T, sky, case)
    t.render(1)
    before = t.read_canvas()
    other = shapes.copy()
    other["material"][:] = 0  # another scene: were it taken, the canvas would change
    too_long = np.append(case["tm"], 0).astype(np.int32)
    out_of_range = case["tm"].copy()
    out_of_range[3] = len(mats)
    below = case["tm"].copy()
    below[3] = -2
    for bad in (too_long, out_of_range, below):
        t.set_triangle_materials(bad)  # after update_scene: fails at the next dispatch
        with pytest.raises(T.SrtError) as e:
            t.render(1)
        assert e.value.code == SRT_ERR_INVALID
        with pytest.raises(T.SrtError) as e:  # and at update_scene, which keeps the previous scene
            t.update_scene(other, tris, mats)
        assert e.value.code == SRT_ERR_INVALID
        t.set_triangle_materials(case["tm"])
        t.clear_canvas()
        t.render(1)
        assert t.last_trace_textured() == 1
        assert bits_equal(t.read_canvas(), before)
    t.close()


# ---- the temporal history ------------------------------------------------------------------------------------------------------------------
def test_setter_drops_the_history(T, sky):
    case = M.tm_case("mesh", "per_face", textured=False)
    t = tracer(T, sky, case, denoise=dict(), temporal=dict())

    def frame():
        t.render(1)
        t.clear_canvas()  # the commit: the frame becomes the history
        return t.read_denoise_history()["valid"]

    assert frame()
    t.set_triangle_materials(M.interleaved(len(case["tm"]), 4))
    assert not t.read_denoise_history()["valid"]
    assert frame()
    t.set_triangle_materials(None)
    assert not t.read_denoise_history()["valid"]
    t.close()


# ---- small fuzz --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz_wants(oracle, sky):
    return {seed: M.oracle_canvas(oracle, sky, M.fuzz_case(seed)) for seed in M.FUZZ_SEEDS}


@pytest.mark.parametrize("accel", [0, 1])
def test_small_fuzz(T, sky, fuzz_wants, accel):
    """40 seeded scenes of two random meshes, random tables with a third of the entries -1, random materials (glass and
    emitters among them), 16x12 at 2 spp, each against the split oracle; one handle, a scene after the other"""
    first = M.fuzz_case(M.FUZZ_SEEDS[0])
    t = tracer(T, sky, first, accel, tm=None)
    bad = []
    for seed in M.FUZZ_SEEDS:
        case = M.fuzz_case(seed)
        t.options["time"] = case["time"]
        t.set_triangle_materials(None)  # (the previous scene's table does not fit this scene)
        t.set_textures(case["images"])
        t.set_material_textures(case["bindings"])
        t.scene_data = R.scene_data(len(case["scn"][0]))
        t.update_scene(*case["scn"])
        t.set_triangle_materials(case["tm"])
        t.clear_canvas()
        t.render(1)
        assert t.last_trace_textured() == 1
        got = t.read_canvas()
        if not bits_equal(got, fuzz_wants[seed]):
            bad.append((seed, differing(got, fuzz_wants[seed])))
    t.close()
    assert not bad, (accel, bad)
