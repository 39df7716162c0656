"""GPU (MI355X): the sky lookup of every trace kernel on skies other than the one 2048 x 1024 picture -- the skies, cameras and
frames of tests/sky_cases.py, whose coverage of the clamp and whose mutants tests/test_sky_cases.py asserts on the CPU. An empty
scene makes the canvas the lookup itself: compared with the numpy restatement of the rule (tests/sky_ref.py) and with the C
oracle. The fuzz lanes carry the small skies through every instantiation and its textured twin, the benchmark scene through
the axis twins. Then the sky replaced on a live handle (smaller, larger, smaller), on a device group, and the refused calls.
Every comparison is exact: canvas bits (NaN equals NaN) and counters."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as FS
import sky_cases as SC
import sky_ref as SR
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu

SKIES = SC.skies()
CAMERAS = SC.cameras()
SRT_ERR_INVALID = 1
YXZ = 2 | (1 << 2) | (3 << 4)  # device_types.h SRT_AXES_PPS_YXZ
# scenes per lane and sky: tests/test_gpu_fuzz_dispatch.py measures 1,400 scenes in 1.96 s (1.4 ms a scene, the oracle's share
# included); a texvar lane's deterministic branches come round in 12 scenes, and by scene 10 every lane has reported each
# (class, textured) pair its full run reports (asserted below against the lanes' own intentions): 12 scenes, some 20 ms a case
LANE_SCENES = 12


@pytest.fixture(scope="module")
def dirs(oracle):
    out = {(c, f): SC.directions(oracle, *CAMERAS[c], *f) for c in CAMERAS for f in SC.FRAMES}
    for d in out.values():
        d.flags.writeable = False
    return out


def empty_tracer(T, sky, w, h):
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.scene_data = SC.scene_data()
    t.update_scene(*SC.empty_scene())
    return t


def one_frame(t, rd, clear=True):
    t.options = rd
    if clear:
        t.clear_canvas()
    t.reset_counters()
    t.trace()
    return t.read_canvas(), t.counters()


# ---- the empty scene: the canvas is the lookup --------------------------------------------------------------------------------
@pytest.mark.parametrize("sky_name", list(SKIES))
def test_empty_scene_is_the_lookup(sky_name, T, oracle, dirs):
    """Every camera and both frame sizes. 1 sample: read_canvas() is the restatement's sky_box + 0 of the pixel's direction (and
    the oracle's frame). 3 samples under a radiance budget of one sample (three batches): the oracle's frame. Both: the oracle's
    sky, paths and nan_pixels -- on the specials sky and under the NaN camera the count of NaN pixels is not 0."""
    sky = SKIES[sky_name]
    sd = SC.scene_data()
    nan_pixels = 0
    for w, h in SC.FRAMES:
        t = empty_tracer(T, sky, w, h)
        try:
            for c, (cam, fov) in CAMERAS.items():
                for spp in (1, 3):
                    t.set_radiance_budget(w * h * 12 if spp == 3 else 0)  # 12 bytes per pixel and sample: batches of one sample
                    got, ctr = one_frame(t, SC.render_data(cam, fov, w, h, spp))
                    want, oc = SC.oracle_frame(oracle, sky, cam, fov, w, h, spp, counters=True)
                    what = (sky_name, c, w, h, spp)
                    assert bits_equal(got, want), (what, FS.differing_pixels(got, want))
                    if spp == 1:
                        rule = SR.frame(sd, sky, dirs[c, (w, h)]).reshape(h, w, 3)
                        assert bits_equal(got[..., :3], rule), (what, FS.differing_pixels(got[..., :3], rule))
                    else:
                        assert t.last_trace_launches()[0] >= 3, what
                    for k in ("sky", "paths", "nan_pixels"):
                        assert ctr[k] == oc[k], (what, k, ctr, oc)
                    assert ctr["sky"] == ctr["paths"] == w * h * spp and ctr["watchdog"] == 0, (what, ctr)
                    nan_pixels += ctr["nan_pixels"]
        finally:
            t.close()
    assert (nan_pixels > 2 * 1841) == (sky_name == "specials")  # the NaN camera's frames: 2 * (768 + 1073) on every sky


# ---- every trace kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky_name", ["3x2", "specials"])
@pytest.mark.parametrize("name", list(FS.LANES))
def test_lanes_on_small_skies(name, sky_name, T, oracle):
    """The fuzz lanes (benign) with a 3 x 2 sky and with the specials sky: mirror and glass bounces send directions all round,
    across the seam and to both poles, in every instantiation and its textured twin. run_lane demands the oracle's canvas and
    counters and the lane's class for every scene; the (class, textured) pairs reported over the short run are all those the
    lane's full run intends, and no lane's planes are axis planes."""
    report = []
    failures, classes, _ = FS.run_lane(T, oracle, SKIES[sky_name], name, False, LANE_SCENES, report=report)
    assert not failures, failures
    assert len(report) == LANE_SCENES
    rng = np.random.RandomState(FS.lane_seed(name, False))
    full = {tuple(FS.LANES[name](rng, False, it)[6]) for it in range(FS.lane_iterations(name))}
    assert {(cls, bool(tex)) for cls, _, tex in report} == {(cls, bool(tex)) for cls, tex in full}, (report, full)
    assert {form for _, form, _ in report} == {0}


def test_lanes_reach_every_kind_of_kernel():
    """Over the lanes' intentions (no device needed): the four classes, the general kernels and the textured twins are all there."""
    kinds = set()
    for name in FS.LANES:
        rng = np.random.RandomState(FS.lane_seed(name, False))
        kinds |= {tuple(FS.LANES[name](rng, False, it)[6]) for it in range(LANE_SCENES)}
    assert {(c, False) for c in (FS.GENERAL, FS.PPS, FS.PPS_SPECULAR, FS.SSS, FS.PPP)} | {(FS.GENERAL, True)} == {(c, bool(x)) for c, x in kinds}


@pytest.mark.parametrize("sky_name", ["3x2", "specials"])
@pytest.mark.parametrize("cls", [FS.PPS, FS.PPS_SPECULAR])
def test_axis_twins_on_small_skies(cls, sky_name, T, oracle):
    """The benchmark scene (planes y, x | plane z | four spheres, a mirror and a glass one among them) runs the axis twin of its
    class: the oracle's canvas and counters on a ragged frame."""
    shapes, tris, mats = S.sphere_scene()
    mats = mats.copy()
    if cls == FS.PPS_SPECULAR:
        mats["specular"][0] = 0.5
    w, h = SC.FRAMES[1]
    rd = R.render_data(w, h, 8, 10, camera_to_world=S.default_camera(), time=4711)
    sd = R.scene_data(len(shapes))
    sky = SKIES[sky_name]
    with np.errstate(all="ignore"):
        want, oc = oracle.render(rd, sd, shapes, tris, mats, sky, counters=True, nthreads=4)
    t = T.Tracer(w, h)
    try:
        t.set_skybox(sky)
        t.scene_data = sd
        t.update_scene(shapes, tris, mats)
        got, ctr = one_frame(t, rd)
        assert (t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured()) == (cls, YXZ, False)
        assert bits_equal(got, want), FS.differing_pixels(got, want)
        assert {k: ctr[k] for k in FS.COUNTERS} == {k: oc[k] for k in FS.COUNTERS} and ctr["watchdog"] == 0
        assert oc["sky"] > w * h  # (paths do end in the sky)
    finally:
        t.close()


# ---- replacing the sky on a live handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["seam", "down"])
def test_sky_replaced_on_a_live_handle(camera, T, oracle, sky):
    """5x7, 1x1, the 2048 x 1024 picture and 3x2 installed in turn on one handle, a trace after each, the canvas never cleared:
    the oracle's accumulation with the same sky per frame. Then the handle's frame alone is that of a fresh handle which has
    only ever seen the 3x2 sky: nothing of a larger, older image is read."""
    w, h = SC.FRAMES[1]
    cam, fov = CAMERAS[camera]
    rd = SC.render_data(cam, fov, w, h, 2)
    order = [SKIES["5x7"], SKIES["1x1"], sky, SKIES["3x2"]]
    t = empty_tracer(T, order[0], w, h)
    fresh = empty_tracer(T, order[-1], w, h)
    try:
        t.clear_canvas()
        want = np.zeros((h, w, 4), np.float32)
        for k, image in enumerate(order):
            t.set_skybox(image)
            got, _ = one_frame(t, rd, clear=False)
            want = SC.oracle_frame(oracle, image, cam, fov, w, h, 2, canvas=want)
            assert bits_equal(got, want), (k, FS.differing_pixels(got, want))
        alone, _ = one_frame(t, rd)
        first, _ = one_frame(fresh, rd)
        assert bits_equal(alone, first), FS.differing_pixels(alone, first)
        assert bits_equal(first, SC.oracle_frame(oracle, order[-1], cam, fov, w, h, 2))
    finally:
        t.close()
        fresh.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_sets_the_sky_on_every_member(world, T, dirs):
    """srt_group_set_skybox with the 5x7 sky on 2 and 3 virtual devices: the single handle's canvas, which is the restatement's."""
    w, h = SC.FRAMES[1]
    sky = SKIES["5x7"]
    single = empty_tracer(T, sky, w, h)
    g = T.TracerGroup(w, h, n_devices=world, devices=[0] * world, rows_per_block=4)
    try:
        g.set_skybox(SKIES["31x13"])  # (replaced below: the members, too, take a smaller image after a larger one)
        g.set_skybox(sky)
        g.scene_data = SC.scene_data()
        g.update_scene(*SC.empty_scene())
        for c in ("seam", "down", "at_-x_z-0"):
            cam, fov = CAMERAS[c]
            rd = SC.render_data(cam, fov, w, h)
            want, _ = one_frame(single, rd)
            g.options = rd
            g.clear_canvas()
            g.render(1)
            got = g.read_canvas()
            assert bits_equal(got, want), (c, FS.differing_pixels(got, want))
            assert bits_equal(got[..., :3], SR.frame(SC.scene_data(), sky, dirs[c, (w, h)]).reshape(h, w, 3)), c
    finally:
        g.close()
        single.close()


def test_refused_images_leave_the_old_sky(T):
    """Width 0, a negative height and a null image are SRT_ERR_INVALID each, and the next frame is still the old sky's."""
    w, h = SC.FRAMES[0]
    cam, fov = CAMERAS["seam"]
    rd = SC.render_data(cam, fov, w, h)
    t = empty_tracer(T, SKIES["5x7"], w, h)
    try:
        before, _ = one_frame(t, rd)
        other = np.ascontiguousarray(SKIES["3x2"])
        ptr = other.ctypes.data_as(C.c_void_p)
        for image, width, height in ((ptr, 0, 2), (ptr, 3, -2), (None, 3, 2)):
            assert t.lib.srt_set_skybox(t._h, image, width, height) == SRT_ERR_INVALID, (width, height)
            after, _ = one_frame(t, rd)
            assert bits_equal(after, before), (width, height)
        t.set_skybox(other)  # (and an accepted image does change the frame)
        changed, _ = one_frame(t, rd)
        assert FS.differing_pixels(changed, before) > w * h // 2
    finally:
        t.close()
