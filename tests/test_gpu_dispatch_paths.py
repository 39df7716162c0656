"""GPU: every way into the trace dispatch (srt_abi.hip srt_trace_fused) gives the same frame. trace() + resolve(),
render(), render_pipelined() + pipeline_flush() over {untextured, textured} x {one launch, sample batches on two streams}
x {denoiser off, on}: canvas, filter result and ARGB bytes bit for bit, the launch counts and the textured flag, and the
same for num_samples = 0 (no trace launch at all: one reduction that still resolves)."""
import numpy as np
import pytest

from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES = 40, 30, 5, 3
# (samples, radiance budget) -> (launches, overlapped), by trace_plan.h plan_batch (tests/test_host_units.py runs it on the
# host). Five samples under the default budget are NOT one launch: a batch above 4 is a multiple of 4 (the reduction's
# 16-byte loads), so they run as 4 + 1 on two streams; four samples are one launch on the handle's stream. Several batches
# alternate between TWO radiance buffers and both must fit the budget: two buffers of two samples give launches of 2, 2 and
# 1 samples, and W * H * 12 * 2 bytes hold two buffers of ONE sample: five launches, none ragged.
BUDGETS = {"default_budget": (SPP, None, (2, True)), "one_launch": (4, None, (1, False)),
           "three_launches": (SPP, W * H * 12 * 2 * 2, (3, True)), "five_launches": (SPP, W * H * 12 * 2, (5, True))}
PLANE_MATERIAL = 2


def scene():
    """two spheres, a plane and one box of 12 triangles, every shape its own material"""
    mats = np.array([R.material(color=(0.9, 0.3, 0.2)), R.material(color=(0.95, 0.95, 0.95), smoothness=0.9, metallic=1.0),
                     R.material(color=(0.8, 0.8, 0.7)), R.material(color=(0.2, 0.5, 0.9), specular=0.3, smoothness=0.5)], R.MATERIAL)
    tris = R.box_triangles()
    shapes = np.array([R.sphere(0, (-1.2, 0.4, 0.0), 0.9), R.sphere(1, (0.9, 0.2, 1.0), 0.7), R.plane(PLANE_MATERIAL, (0.0, -0.5, 0.0), (0.0, 1.0, 0.0)),
                       R.model(3, tris, 0, 12, R.mat_mul(R.translate((1.6, 0.3, -1.5)), R.scale_matrix((0.7, 0.8, 0.6))))], R.SHAPE)
    return shapes, tris, mats


def handle(T, sky, textured, budget, denoise, spp=SPP):
    """a handle over scene(), fed the same way whatever is called on it afterwards"""
    shapes, tris, mats = scene()
    t = T.Tracer(W, H)
    t.set_skybox(sky)
    t.options = R.render_data(W, H, spp, BOUNCES, camera_to_world=S.default_camera(), time=2718)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    if textured:  # one 4x4 image on the plane's material
        t.set_textures([np.random.default_rng(5).uniform(0.05, 1.0, (4, 4, 4)).astype(np.float32)])
        b = np.zeros(len(mats), R.MATERIAL_TEXTURE)
        for i in range(len(mats)):
            b[i] = R.material_texture(0 if i == PLANE_MATERIAL else -1, 0, 3.0, 2.0)  # bilinear
        t.set_material_textures(b)
    if budget is not None:
        t.set_radiance_budget(budget)
    if denoise:
        t.set_denoise(iterations=2)
    t.clear_canvas()
    return t


def frame_by(T, sky, route, textured, budget, denoise, spp=SPP):
    """one frame by `route` on a fresh handle -> dict(canvas, argb, launches, textured[, denoised])"""
    t = handle(T, sky, textured, budget, denoise, spp)
    if route == "trace_resolve":
        t.trace()
        launches, tex = t.last_trace_launches(), t.last_trace_textured()
        if denoise:
            t.resolve_denoised(1)
        else:
            t.resolve(1)
        argb = t.read_argb().reshape(-1).copy()
    elif route == "trace_plain_resolve":  # the plain resolve, whatever the denoiser's state
        t.trace()
        launches, tex = t.last_trace_launches(), t.last_trace_textured()
        t.resolve(1)
        argb = t.read_argb().reshape(-1).copy()
    elif route == "render":
        argb = t.render(1).copy()
        launches, tex = t.last_trace_launches(), t.last_trace_textured()
    else:
        argb = np.zeros(W * H * 4, np.uint8)
        assert t.render_pipelined(1, argb) == -1  # nothing to deliver yet
        launches, tex = t.last_trace_launches(), t.last_trace_textured()
        assert t.pipeline_flush(argb) == 0
    out = dict(canvas=t.read_canvas(), argb=argb, launches=launches, textured=tex)
    if denoise and route != "trace_plain_resolve":
        out["denoised"] = t.read_denoised()
    t.close()
    return out


@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoised"])
@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("textured", [False, True], ids=["untextured", "textured"])
def test_every_route_gives_the_same_frame(T, sky, textured, budget, denoise):
    spp, nbytes, want_launches = BUDGETS[budget]
    frames = {route: frame_by(T, sky, route, textured, nbytes, denoise, spp) for route in ("trace_resolve", "render", "pipelined")}
    want = frames["render"]
    assert np.isfinite(want["canvas"]).all() and want["canvas"][..., :3].max() > 0 and want["argb"].reshape(-1, 4)[:, 1:].any()
    for route, got in frames.items():
        assert got["launches"] == want_launches, (route, got["launches"])
        assert got["textured"] == textured, route
        assert bits_equal(got["canvas"], want["canvas"]), route
        assert np.array_equal(got["argb"], want["argb"]), (route, int((got["argb"] != want["argb"]).sum()))
        if denoise:
            assert bits_equal(got["denoised"], want["denoised"]), route


def test_the_texture_and_the_filter_show(T, sky):
    """the matrix above compares like with like; its cells do differ from one another"""
    plain = frame_by(T, sky, "render", False, None, False)
    tex = frame_by(T, sky, "render", True, None, False)
    den = frame_by(T, sky, "render", False, None, True)
    assert not bits_equal(tex["canvas"], plain["canvas"])
    assert bits_equal(den["canvas"], plain["canvas"]) and not np.array_equal(den["argb"], plain["argb"])


@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoised"])
@pytest.mark.parametrize("textured", [False, True], ids=["untextured", "textured"])
def test_no_samples_through_every_route(T, sky, textured, denoise):
    """num_samples = 0: no trace launch, one reduction that adds 0 / 0 to every pixel and, in the render calls, resolves"""
    want = frame_by(T, sky, "render", textured, None, denoise, spp=0)
    assert np.isnan(want["canvas"][..., :3]).all() and want["launches"] == (0, False)
    for route in ("trace_plain_resolve", "trace_resolve", "pipelined"):
        got = frame_by(T, sky, route, textured, None, denoise, spp=0)
        assert got["launches"] == (0, False) and got["textured"] == textured, route
        assert bits_equal(got["canvas"], want["canvas"]), route
        assert np.array_equal(got["argb"], want["argb"]), route
