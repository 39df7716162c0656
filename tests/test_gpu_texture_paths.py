"""GPU: albedo textures at full depth. Every canvas here is the textured CPU oracle's (oracle/srt_oracle.c
orc_render_textured, earned by tests/test_oracle_textures.py) bit for bit: spatially varying textures, both filters, negative
and non-integer scales, ten bounces, so a wrong texel at ANY hit of a path -- a hit record out of the wave's queue, out of a
suspended scan or the ray pool, a back face inside glass, a triangle reached by a bounce ray, the BVH's leaf reference --
changes bits. The cases are tests/texture_cases.py path_case(); every (case, frame) rendered here is listed in its GPU_VIEWS,
and tests/test_oracle_textures.py asserts on each of them, both filters, that at least a fifth of the paths read a texel
beyond their first hit. The floor's coat carries two texels whose mix(texel, 1, 1) is not 1.0f, so the texel's bits count at
specular bounces too (asserted there as well)."""
import numpy as np
import pytest

import texture_cases as TC
import texture_ref as TR
from conftest import bits_equal
from gpu_harness import T, make  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu
F = np.float32
FILTERS = [TR.LINEAR, TR.NEAREST]
FRAMES = TC.FRAMES


def tracer(T, sky, case, accel=0, denoise=None):
    t = make(T, sky, case["scn"], case["w"], case["h"], spp=case["spp"], accel=accel, time=case["time"], cam=case["cam"], denoise=denoise)
    t.options["num_bounces"] = case["bounces"]
    bind(t, case)
    t.clear_canvas()
    return t


def bind(t, case):
    t.set_textures(case["images"])
    t.set_material_textures(case["bindings"])
    t.set_triangle_uvs(case["uvs"])


def gpu_canvas(T, sky, case, accel=0, budget=None):
    t = tracer(T, sky, case, accel)
    if budget is not None:
        t.set_radiance_budget(budget)
    t.render(1)
    out = t.read_canvas(), t.options.copy(), t.scene_data.copy(), t.last_trace_launches()
    assert t.last_trace_textured()
    t.close()
    return out


def check(T, sky, oracle, case, accel=0, what=None):
    got, rd, sd, _ = gpu_canvas(T, sky, case, accel)
    want = TC.oracle_path_canvas(oracle, sky, case, rd, sd)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert bits_equal(got, want), (what, accel, f"{bad} of {got.shape[0] * got.shape[1]} pixels differ")


# ---- spheres and planes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", ["material", "material_pad", "material_nospec", "material_nospec_pad"])
def test_material_scene(T, sky, oracle, name, filt, w, h):
    """Mirror, glass (back faces: the sphere's UV takes the unflipped normal), rough metal, a specular coat, a textured emitter
    and a plane without a frame; scene records in LDS and (80 padding materials) in global memory; with a specular coat
    (mix3(texel, 1, is_specular)) and with every specular probability 0 (the `mask * texel` shortcut, whose flag looks at
    the material colours only)."""
    check(T, sky, oracle, TC.path_case(name, filt, w=w, h=h), what=(name, filt, w, h))


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("with_uvs", [True, False])
@pytest.mark.parametrize("filt", FILTERS)
def test_mesh_scene(T, sky, oracle, filt, with_uvs, accel, w, h):
    """Rotated, non-uniformly scaled boxes, one of glass, over a mirror floor, two instances over one triangle range with
    different textures: barycentrics from a bounce ray's position, from outside and inside; array scan and BVH."""
    check(T, sky, oracle, TC.path_case("mesh", filt, with_uvs, w=w, h=h), accel, what=("mesh", filt, with_uvs))


# ---- big models ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("filt", FILTERS)
def test_big_models(T, sky, oracle, filt, accel):
    """Models of 128 and more triangles, glass and mirror, every material textured: the array scan suspends their rays (the
    hit records then come from the scan queue), the BVH hands back a leaf-block reference; with the triangle counters
    (the textured COUNT_TRIS twins) and without. Counters as tests/test_gpu_large_scene.py."""
    case = TC.path_case("big", filt, with_uvs=(filt == TR.LINEAR))
    shapes, tris, mats = case["scn"]
    t = tracer(T, sky, case, accel)
    rd, sd = t.options.copy(), t.scene_data.copy()
    want, oc = TC.oracle_path_canvas(oracle, sky, case, rd, sd, counters=True)
    for count in (True, False):
        t.count_triangles(count)
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        got, c = t.read_canvas(), t.counters()
        assert t.last_trace_textured()
        assert bits_equal(got, want), (filt, accel, count, int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum()))
        for k in ("paths", "rays", "sky") + (("tri_tests", "tri_pass_u") if count and accel == 0 else ()):
            assert c[k] == oc[k], (k, c[k], oc[k])
        assert c["watchdog"] == 0
    if accel == 0:
        assert t.debug_counters()["scans"] > 0  # the suspended-scan route carried textured hits
    t.close()


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
ROUTE_CASES = [("material", 0), ("mesh", 1)]


@pytest.fixture(scope="module")
def route_wants(oracle, sky):
    return {name: TC.oracle_path_canvas(oracle, sky, TC.path_case(name, TR.LINEAR)) for name, _ in ROUTE_CASES}


@pytest.mark.parametrize("name,accel", ROUTE_CASES)
def test_sample_batches(T, sky, route_wants, name, accel):
    case = TC.path_case(name, TR.LINEAR)
    """Two radiance buffers of ONE sample each (12 bytes per pixel and sample) are all the budget holds: the four samples
    run as four launches that overlap on two streams (trace_plan.h plan_batch; tests/test_gpu_dispatch_paths.py)."""
    got, _, _, launches = gpu_canvas(T, sky, case, accel, budget=case["w"] * case["h"] * 12 * 2)
    assert launches == (4, True)
    assert bits_equal(got, route_wants[name])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,accel", ROUTE_CASES)
def test_row_partitions(T, sky, route_wants, name, accel, world):
    case = TC.path_case(name, TR.LINEAR)
    full = np.zeros_like(route_wants[name])
    for rank in range(world):
        t = tracer(T, sky, case, accel)
        t.set_partition(rank, world, 3)
        t.clear_canvas()
        t.render(1)
        part = t.read_canvas()
        assert t.last_trace_textured()
        for r in range(t.owned_rows):
            full[T.global_row(case["h"], rank, world, 3, r)] = part[r]
        t.close()
    assert bits_equal(full, route_wants[name])


@pytest.mark.parametrize("name,accel", ROUTE_CASES)
def test_device_group(T, sky, route_wants, name, accel):
    case = TC.path_case(name, TR.LINEAR)
    rd, _ = TC.case_render_data(case)
    g = T.TracerGroup(case["w"], case["h"], n_devices=3, devices=[0] * 3, rows_per_block=3)
    g.set_skybox(sky)
    g.set_acceleration(accel)
    g.options = rd
    g.scene_data = R.scene_data(len(case["scn"][0]))
    bind(g, case)
    g.update_scene(*case["scn"])
    g.clear_canvas()
    g.render(1)
    got = g.read_canvas()
    g.close()
    assert bits_equal(got, route_wants[name])


# ---- the feature pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [1, 3, 8])
@pytest.mark.parametrize("name,accel", [("material", 0), ("big", 0), ("big", 1)])
def test_albedo_guide(T, sky, oracle, name, accel, fs):
    case = dict(TC.path_case(name, TR.LINEAR), spp=8)
    shapes, tris, mats = case["scn"]
    t = tracer(T, sky, case, accel, denoise=dict(feature_samples=fs, iterations=0))
    t.render(1)
    inp, rd, sd = t.read_denoise_inputs(), t.options.copy(), t.scene_data.copy()
    t.close()
    table = TC.oracle_table(case["scn"], case["images"], case["bindings"], case["uvs"])
    nd, ah = oracle.features_textured(rd, sd, shapes, tris, mats, table, fs)
    assert bits_equal(inp["normal_depth"], nd)
    assert bits_equal(inp["albedo_hits"], ah), (name, accel, fs)
