"""GPU (MI355X): the scene classes of the sphere / plane trace kernel (kernels.hip "SCENE CLASSES"). A scene of one block
group whose layout is on device_types.h's SRT_SCENE_CLASS_LIST runs a kernel compiled for it; every other scene, and every
dispatch with show_normals, no bounces, textures or triangle counting, runs the general kernel. Whichever kernel runs, the
canvas and the counters are the CPU oracle's bit for bit -- and every case asserts WHICH kernel ran (Tracer.last_trace_class),
so that nothing here passes by always falling back."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 64, 8
GENERAL, PPS, PPS_SPECULAR, SSS, PPP = 0, 1, 2, 3, 4  # device_types.h SRT_SCENE_CLASS_LIST


def stack(items, dtype):
    a = np.zeros(len(items), dtype)
    for i, it in enumerate(items):
        a[i] = it
    return a


def spheres(n):
    """n spheres in rows in front of the camera, the sphere scene's seven materials in turn (glass, metal and a light among them)"""
    out = []
    for i in range(n):
        x, y, z = -3.0 + 2.0 * (i % 4), -0.4 + 1.3 * ((i // 4) % 2), -1.0 - 1.7 * (i // 4) - 0.3 * (i % 3)
        out.append(R.sphere(i % 7, (x, y, z), 0.55 + 0.07 * (i % 5)))
    return out


def planes6():
    """a closed room of six planes around the camera"""
    return [R.plane(0, (0, -1, 0), (0, 1, 0)), R.plane(6, (0, 5, 0), (0, -1, 0)), R.plane(1, (-4, 0, 0), (1, 0, 0)),
            R.plane(2, (4, 0, 0), (-1, 0, 0)), R.plane(5, (0, 0, -6), (0, 0, 1)), R.plane(3, (0, 0, 9), (0, 0, -1))]


def scene(name):
    """-> shapes, tris, mats, class the library must choose (with bounces, without show_normals)"""
    shapes, tris, mats = S.sphere_scene()
    shapes, mats = shapes.copy(), mats.copy()
    if name == "base":  # two planes | one plane | four spheres
        return shapes, tris, mats, PPS
    if name == "spheres12":  # the most spheres one group holds
        return stack(spheres(12), R.SHAPE), tris, mats, SSS
    if name == "planes6":  # the most planes one group holds
        return stack(planes6(), R.SHAPE), tris, mats, PPP
    if name == "spheres12_planes6":  # six blocks: two groups
        return stack(spheres(12) + planes6(), R.SHAPE), tris, mats, GENERAL
    if name == "spheres13":  # four blocks: two groups
        return stack(spheres(13), R.SHAPE), tris, mats, GENERAL
    if name == "spheres3":  # one group, but a layout no class is compiled for
        return stack(spheres(3), R.SHAPE), tris, mats, GENERAL
    if name == "no_material":
        shapes["material"][4] = -1
        return shapes, tris, mats, GENERAL
    if name == "specular":
        mats["specular"][1] = 0.5
        mats["specular"][3] = 1.0
        return shapes, tris, mats, PPS_SPECULAR
    if name == "probability_above_1":  # no integer threshold for it: the float compares of the general kernel
        mats["metallic"][2] = 1.5
        return shapes, tris, mats, GENERAL
    if name == "model":
        return (*S.mixed_test_scene(), GENERAL)
    raise ValueError(name)


SCENES = ["base", "spheres12", "planes6", "spheres12_planes6", "spheres13", "spheres3", "no_material", "specular",
          "probability_above_1", "model"]
FAST = {"base": PPS, "spheres12": SSS, "planes6": PPP, "specular": PPS_SPECULAR}  # every class the library compiles is chosen somewhere


def options(bounces=10, show_normals=False, time=4711, spp=SPP, w=W, h=H):
    return R.render_data(w, h, spp, bounces, camera_to_world=S.default_camera(), time=time, show_normals=show_normals)


def tracer(T, sky, scn, rd):
    shapes, tris, mats = scn
    t = T.Tracer(int(rd["width"]), int(rd["height"]))
    t.set_skybox(sky)
    t.options = rd.copy()
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t


def check_frame(t, oracle, sky, scn, cls, what):
    """one cleared frame of t's options over scn: the class, the canvas and the counters"""
    shapes, tris, mats = scn
    t.clear_canvas()
    t.reset_counters()
    t.trace()
    got, c = t.read_canvas(), t.counters()
    assert t.last_trace_class() == cls, (what, t.last_trace_class(), cls)
    want, oc = oracle.render(t.options, R.scene_data(len(shapes)), shapes, tris, mats, sky, counters=True)
    assert bits_equal(got, want), what
    for k in ("paths", "rays", "sky", "nan_pixels"):
        assert c[k] == oc[k], (what, k, c, oc)
    assert c["watchdog"] == 0, what


@pytest.mark.parametrize("name", SCENES)
def test_scene_decides_the_class(name, T, sky, oracle):
    *scn, cls = scene(name)
    assert cls == FAST.get(name, GENERAL)
    t = tracer(T, sky, scn, options())
    check_frame(t, oracle, sky, scn, cls, name)
    t.close()


@pytest.mark.parametrize("bounces,show_normals,fast", [(0, False, False), (1, False, True), (10, True, False), (1, True, False)])
def test_options_decide_the_class(bounces, show_normals, fast, T, sky, oracle):
    *scn, cls = scene("base")
    t = tracer(T, sky, scn, options(bounces, show_normals))
    check_frame(t, oracle, sky, scn, cls if fast else GENERAL, (bounces, show_normals))
    t.close()


def test_triangle_counting_runs_the_general_kernel(T, sky, oracle):
    *scn, cls = scene("base")
    t = tracer(T, sky, scn, options())
    t.count_triangles(True)
    check_frame(t, oracle, sky, scn, GENERAL, "count_triangles on")
    t.count_triangles(False)
    check_frame(t, oracle, sky, scn, cls, "count_triangles off")
    t.close()


def test_class_changes_on_a_live_handle(T, sky, oracle):
    """fast scene, general scene, fast scene through update_scene on one Tracer (another fast class in between), and show_normals
    toggled between two renders: every frame is the oracle's, from the kernel of its class"""
    t = None
    for name in ("base", "spheres13", "spheres12", "model", "planes6", "base"):
        *scn, cls = scene(name)
        if t is None:
            t = tracer(T, sky, scn, options())
        else:
            t.scene_data = R.scene_data(len(scn[0]))
            t.update_scene(*scn)
        check_frame(t, oracle, sky, scn, cls, name)
    for show, want_cls in ((True, GENERAL), (False, PPS), (True, GENERAL), (False, PPS)):
        t.options["show_normals"] = 1 if show else 0
        t.options["time"] = np.uint32(int(t.options["time"]) + 1)
        check_frame(t, oracle, sky, scn, want_cls, f"show_normals {show}")
    t.close()


@pytest.mark.parametrize("name", sorted(FAST))
def test_sample_batches_are_invisible(name, T, sky, oracle):
    """a radiance budget too small for the dispatch (about three batches, one ragged; then one sample per batch)"""
    *scn, cls = scene(name)
    rd = options(spp=7)
    want = oracle.render(rd, R.scene_data(len(scn[0])), *scn, sky)
    for budget in (W * H * 12 * 2, 1):
        t = tracer(T, sky, scn, rd)
        t.set_radiance_budget(budget)
        t.trace()
        assert t.last_trace_class() == cls
        assert bits_equal(t.read_canvas(), want), (name, budget)
        assert t.counters()["watchdog"] == 0
        t.close()


@pytest.mark.parametrize("name", sorted(FAST))
def test_interleaved_partition_equals_the_whole_frame(name, T, sky, oracle):
    """rank 1 of 3, blocks of 8 rows: its packed rows are the whole frame's rows, from the class's kernel"""
    *scn, cls = scene(name)
    rd = options()
    want = oracle.render(rd, R.scene_data(len(scn[0])), *scn, sky)
    for rank in range(3):
        t = tracer(T, sky, scn, rd)
        t.set_partition(rank, 3, 8)
        t.clear_canvas()
        t.trace()
        assert t.last_trace_class() == cls
        part = t.read_canvas()
        assert t.owned_rows > 0
        for r in range(t.owned_rows):
            assert bits_equal(part[r], want[T.global_row(H, rank, 3, 8, r)]), (name, rank, r)
        t.close()


def test_group_of_two_virtual_devices(T, sky, oracle):
    *scn, cls = scene("base")
    rd = options()
    want = oracle.render(rd, R.scene_data(len(scn[0])), *scn, sky)
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
    g.set_skybox(sky)
    g.options = rd.copy()
    g.scene_data = R.scene_data(len(scn[0]))
    g.update_scene(*scn)
    g.clear_canvas()
    g.render(1)
    got = g.read_canvas()
    for i in range(2):
        member, out = C.c_void_p(g.lib.srt_group_tracer(g._g, i)), C.c_int(-1)
        assert g.lib.srt_last_trace_class(member, C.byref(out)) == 0
        assert out.value == cls, (i, out.value)
    g.close()
    assert bits_equal(got, want)
