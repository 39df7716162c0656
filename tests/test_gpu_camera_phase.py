"""GPU (MI355X): the camera phases of the scene-class trace kernels (device_intersect.h "CAMERA PHASES"). An EXTEND phase whose rays
are all fresh camera rays starts from numbers the wave made once from the shapes and the camera's origin, and skips, by wave
vote, spheres and planes that no ray of the phase can hit. None of it may change a bit: every case compares the canvas and the
path / ray / sky / NaN counters with the CPU oracle, asserts WHICH kernel ran (Tracer.last_trace_class) and asserts that camera
phases were counted (debug_counters()["camera_phases"] > 0; == 0 for the general kernel, which has none).

The frames are at most 64x48. The cases aim at how a phase's 64 lanes are laid out over pixels, at launches that begin at
another sample or own other rows, at cameras that put the hoisted numbers and the votes at their edges, and at hostile shapes
that stay inside a class. A CPU test (no marker) holds the hostile scenes to the cap of tests/test_fuzz_lanes.py."""
import numpy as np
import pytest

import fuzz_scenes as FS
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

GENERAL, PPS, PPS_SPECULAR, SSS, PPP = 0, 1, 2, 3, 4  # device_types.h SRT_SCENE_CLASS_LIST
COUNTERS = ("paths", "rays", "sky", "nan_pixels")
F = np.float32


def base_scene():
    shapes, tris, mats = S.sphere_scene()  # two planes | one plane | four spheres: the benchmark's scene, class PPS
    return shapes.copy(), tris, mats.copy()


def options(w, h, spp, cam=None, fov=1.0, bounces=10, time=4711):
    return R.render_data(w, h, spp, bounces, fov_scale=fov, camera_to_world=S.default_camera() if cam is None else cam, time=time)


def tracer(T, sky, scn, rd, sd=None):
    shapes, tris, mats = scn
    t = T.Tracer(int(rd["width"]), int(rd["height"]))
    t.set_skybox(sky)
    t.options = rd.copy()
    t.scene_data = R.scene_data(len(shapes)) if sd is None else sd
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t


def oracle_frame(oracle, sky, scn, rd, sd=None):
    shapes, tris, mats = scn
    with np.errstate(all="ignore"):
        return oracle.render(rd, R.scene_data(len(shapes)) if sd is None else sd, shapes, tris, mats, sky, counters=True, nthreads=4)


def trace_and_check(t, want, oc, cls, what):
    """one cleared frame: class, canvas bits, counters, watchdog; camera phases counted exactly when a class kernel ran.
    -> the diagnostics"""
    t.clear_canvas()
    t.reset_counters()
    t.trace()
    got, c, d = t.read_canvas(), t.counters(), t.debug_counters()
    print(what, {k: c[k] for k in COUNTERS}, "camera phases", d["camera_phases"], "rays in them", d["camera_phase_rays"])
    assert t.last_trace_class() == cls, (what, t.last_trace_class(), cls)
    assert bits_equal(got, want), (what, FS.differing_pixels(got, want))
    for k in COUNTERS:
        assert c[k] == oc[k], (what, k, c, oc)
    assert c["watchdog"] == 0, what
    if cls == GENERAL:
        assert d["camera_phases"] == 0 and d["camera_phase_rays"] == 0, (what, d)
    else:
        assert d["camera_phases"] > 0, (what, d)
        assert 0 < d["camera_phase_rays"] <= c["paths"], (what, d)  # every ray of such a phase is a path's first
    return d


# ---- lane layouts ---------------------------------------------------------------------------------------------------------------
# 64 and 1024 spp: a phase is one pixel. 3, 16, 100: phases straddle pixels and rows. 1 spp: 64 different pixels per phase, the
# votes seldom skip and must not matter. 1x1x5 and 5x3x7: fewer than 64 items, and a count that is no multiple of 64: the last
# phases mix camera and bounce rays and the flag must fall back to the general form.
LAYOUTS = [(48, 32, 1), (48, 32, 3), (48, 32, 16), (48, 32, 64), (48, 32, 100), (8, 4, 1024), (1, 1, 5), (5, 3, 7)]
_base_want = {}


def base_want(oracle, sky, w, h, spp):
    """the oracle's frame of the benchmark scene under the default camera, computed once per shape"""
    if (w, h, spp) not in _base_want:
        _base_want[w, h, spp] = oracle_frame(oracle, sky, base_scene(), options(w, h, spp))
    return _base_want[w, h, spp]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", LAYOUTS)
def test_lane_layouts(w, h, spp, T, sky, oracle):
    want, oc = base_want(oracle, sky, w, h, spp)
    t = tracer(T, sky, base_scene(), options(w, h, spp))
    trace_and_check(t, want, oc, PPS, (w, h, spp))
    t.close()


# ---- batches and partitions -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sample_batches_start_at_a_later_sample(T, sky, oracle):
    """a radiance budget for 34 of the 100 samples: three batches, first_sample 0, 34, 68"""
    w, h, spp = 48, 32, 100
    want, oc = base_want(oracle, sky, w, h, spp)
    t = tracer(T, sky, base_scene(), options(w, h, spp))
    t.set_radiance_budget(w * h * 12 * 34)
    trace_and_check(t, want, oc, PPS, "three batches")
    assert t.last_trace_launches()[0] >= 3
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_partitions_own_other_rows(world, T, sky, oracle):
    """every rank of a row partition in 8-row blocks: its packed rows are the oracle's rows, its counters add up to the oracle's"""
    w, h, spp = 48, 32, 100
    want, oc = base_want(oracle, sky, w, h, spp)
    total = dict.fromkeys(("paths", "rays", "sky"), 0)
    for rank in range(world):
        t = tracer(T, sky, base_scene(), options(w, h, spp))
        t.set_partition(rank, world, 8)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        assert t.last_trace_class() == PPS
        part, c, d = t.read_canvas(), t.counters(), t.debug_counters()
        assert t.owned_rows > 0 and c["watchdog"] == 0
        assert d["camera_phases"] > 0, (world, rank, d)
        for r in range(t.owned_rows):
            assert bits_equal(part[r], want[T.global_row(h, rank, world, 8, r)]), (world, rank, r)
        for k in total:
            total[k] += c[k]
        t.close()
    assert total == {k: oc[k] for k in total}, (world, total, oc)


# ---- cameras aimed at the hoisted numbers and the votes ---------------------------------------------------------------------------
def look_along(pos, forward):
    """a camera matrix of the test's own: at pos, looking along `forward` (the rays leave along minus the third column)"""
    f = np.asarray(forward, np.float64)
    f = f / np.sqrt((f * f).sum())
    r = np.cross(f, (0.0, 1.0, 0.0))
    r = r / np.sqrt((r * r).sum())
    u = np.cross(r, f)
    m = np.eye(4, dtype=F)
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = r, u, -f, pos
    return m


def edited(cam, row, col, value):
    cam = cam.copy()
    cam[row, col] = value
    return cam


def flipped_floor():
    """the benchmark scene with the floor's normal pointing down: from x > 0, z > 0 on the floor its num is -0, not +0"""
    shapes, tris, mats = base_scene()
    shapes["plane_normal"][0] = (0, -1, 0)
    return shapes, tris, mats


# name -> (scene, camera, fov scale, what the oracle's counters must show: "hits" = camera rays hit a shape for at least a quarter
# of them, "away" = no ray hits anything, None = not a finite camera)
CAMERAS = {
    # the origin exactly on a plane: num = +0 (the quotient is +-0 by the sign of denom: the -0 acceptance, and behind it the
    # spheres' is_neg_zero(tmin) slow path); with the normal flipped, num = -0
    "on_floor": (base_scene, R.camera_matrix((1.0, -1.0, 5.0), 0.0, 0.0), 1.0, "hits"),
    "on_floor_num_neg0": (flipped_floor, R.camera_matrix((1.0, -1.0, 5.0), 0.0, 0.0), 1.0, "hits"),
    "on_wall": (base_scene, R.camera_matrix((-4.0, 0.5, 5.0), 0.0, 0.0), 1.0, "hits"),
    "sphere_centre": (base_scene, R.camera_matrix((-2.0, 0.0, -1.0), 0.0, 0.0), 1.0, "hits"),  # L = 0
    "inside_sphere": (base_scene, R.camera_matrix((-2.5, 0.3, -0.5), 0.3, -0.2), 1.0, "hits"),
    "on_sphere_surface": (base_scene, R.camera_matrix((-2.0, 0.0, 0.5), 0.0, 0.0), 1.0, "hits"),  # c = 0
    "far_away": (base_scene, R.camera_matrix((0.0, 0.5, 1e20), 0.0, 0.0), 1.0, "hits"),  # L*L overflows: c = inf
    "nan_origin": (base_scene, edited(S.default_camera(), 3, 0, np.nan), 1.0, None),
    "inf_origin": (base_scene, edited(S.default_camera(), 3, 1, np.inf), 1.0, None),
    "inf_rotation": (base_scene, edited(S.default_camera(), 0, 0, np.inf), 1.0, None),  # inf * 0: NaN directions
    # up and away from the floor, the wall and the back wall, the spheres behind: every vote skips
    "looks_away": (base_scene, look_along((0.0, 0.5, 5.0), (1.0, 1.0, 1.0)), 0.3, "away"),
    "only_planes": (base_scene, R.camera_matrix((3.0, 0.5, -5.0), 0.0, 0.0), 1.0, "hits"),  # the spheres are behind the camera
    "one_sphere_fills_the_frame": (base_scene, R.camera_matrix((-2.0, 0.0, 1.2), 0.0, 0.0), 0.3, "hits"),
}
CAM_W, CAM_H = 32, 24


def camera_case(name, spp):
    make, cam, fov, claim = CAMERAS[name]
    return make(), options(CAM_W, CAM_H, spp, cam, fov), claim


def check_claim(oracle, sky, scn, rd, claim, oc, what):
    """on the oracle's counters: the camera is what the case says it is"""
    if claim == "away":
        assert oc["rays"] == oc["paths"] == oc["sky"], (what, oc)
    elif claim == "hits":
        first = rd.copy()
        first["num_bounces"] = 1  # one ray per path: those that did not reach the sky hit a shape
        _, c1 = oracle_frame(oracle, sky, scn, first)
        assert c1["rays"] == c1["paths"] and (c1["paths"] - c1["sky"]) * 4 >= c1["paths"], (what, c1)


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_cameras_are_what_they_claim(name, sky, oracle):
    """CPU: the finite cameras below look at what they are meant to look at (both sample counts)"""
    for spp in (64, 70):
        scn, rd, claim = camera_case(name, spp)
        _, oc = oracle_frame(oracle, sky, scn, rd)
        check_claim(oracle, sky, scn, rd, claim, oc, (name, spp))


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [64, 70])
@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_cameras(name, spp, T, sky, oracle):
    scn, rd, claim = camera_case(name, spp)
    want, oc = oracle_frame(oracle, sky, scn, rd)
    t = tracer(T, sky, scn, rd)
    trace_and_check(t, want, oc, PPS, (name, spp))
    t.close()


# ---- hostile shapes inside the class ------------------------------------------------------------------------------------------------
# 50 hostile scenes from each of the four in-class lanes of tests/fuzz_scenes.py (both NO_SPEC values, all four layouts) at 16x16,
# spp drawn from {1, 5, 64, 70}: radii 0 / negative / NaN / 1e20 / 2^-41 / 2^41, zero and huge plane normals, cameras inside
# spheres and behind planes.
HOSTILE_PER_LANE = 50
HOSTILE_SEED = 20261  # (held to the cap by test_hostile_scenes_still_show_something below: 6, 10, 7, 12 of 50)
_hostile = {}


def hostile_scenes(name):
    if name not in _hostile:
        rng = np.random.RandomState(HOSTILE_SEED + sorted(FS.CLASS_LANES).index(name))
        out = []
        for _ in range(HOSTILE_PER_LANE):
            shapes, tris, mats, cam, rd, sd = FS.class_scene(rng, FS.CLASS_LANES[name], True, 16, 16)
            rd["num_samples"] = int(rng.choice([1, 5, 64, 70]))
            out.append((shapes, tris, mats, rd, sd))
        _hostile[name] = out
    return _hostile[name]


_hostile_want = {}


def hostile_want(oracle, sky, name):
    if name not in _hostile_want:
        _hostile_want[name] = [oracle_frame(oracle, sky, (shapes, tris, mats), rd, sd) for shapes, tris, mats, rd, sd in hostile_scenes(name)]
    return _hostile_want[name]


@pytest.mark.parametrize("name", sorted(FS.CLASS_LANES))
def test_hostile_scenes_still_show_something(name, sky, oracle):
    """CPU: the cap of tests/test_fuzz_lanes.py for the seeds used here: at most a quarter of a lane's hostile scenes have more
    than half their pixels NaN or exactly the sky's value; every scene is of the lane's class by the restatement"""
    blank = 0
    for (shapes, tris, mats, rd, sd), (want, oc) in zip(hostile_scenes(name), hostile_want(oracle, sky, name)):
        assert FS.expected_class(shapes, mats, rd) == FS.CLASS_LANES[name]
        empty_sd = sd.copy()
        empty_sd["num_shapes"] = 0
        with np.errstate(all="ignore"):
            nothing = oracle.render(rd, empty_sd, shapes[:0], tris, mats, sky, nthreads=4)
        nan = np.isnan(want[..., :3]).any(axis=-1)
        only_sky = (want.view(np.uint32) == nothing.view(np.uint32)).all(axis=-1)
        blank += int((nan | only_sky).mean() > 0.5)
    print(f"{name}: {blank} of {HOSTILE_PER_LANE} hostile scenes mostly NaN or sky")
    assert blank <= HOSTILE_PER_LANE // 4, (name, blank)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FS.CLASS_LANES))
def test_hostile_shapes_inside_the_class(name, T, sky, oracle):
    cls = FS.CLASS_LANES[name]
    t = T.Tracer(16, 16)
    t.set_skybox(sky)
    bad = []
    try:
        for it, ((shapes, tris, mats, rd, sd), (want, oc)) in enumerate(zip(hostile_scenes(name), hostile_want(oracle, sky, name))):
            t.options, t.scene_data = rd, sd
            t.update_scene(shapes, tris, mats)
            t.clear_canvas()
            t.reset_counters()
            t.trace()
            got, c, d = t.read_canvas(), t.counters(), t.debug_counters()
            ctr = {k: (c[k], oc[k]) for k in COUNTERS if c[k] != oc[k]}
            if t.last_trace_class() != cls or not bits_equal(got, want) or ctr or c["watchdog"] != 0 or d["camera_phases"] == 0:
                bad.append((it, t.last_trace_class(), FS.differing_pixels(got, want), ctr, c["watchdog"], d["camera_phases"]))
    finally:
        t.close()
    assert not bad, (name, bad)


# ---- control: the general kernel has no camera phases ------------------------------------------------------------------------------
def near_misses():
    """one benign near miss per class that must run the general kernel"""
    rng = np.random.RandomState(4242)
    found, it = {}, 0
    while len(found) < 4 and it < 400:
        shapes, tris, mats, cam, rd, sd, expected, extra = FS.near_miss_lane(rng, False, it)
        if expected[0] == GENERAL and extra["base"] not in found:
            found[extra["base"]] = (shapes, tris, mats, rd, sd, extra["what"])
        it += 1
    return found


@pytest.mark.gpu
def test_near_misses_run_the_general_kernel_without_camera_phases(T, sky, oracle):
    found = near_misses()
    assert sorted(found) == [PPS, PPS_SPECULAR, SSS, PPP]
    for base, (shapes, tris, mats, rd, sd, what) in sorted(found.items()):
        assert FS.expected_class(shapes, mats, rd) == GENERAL
        want, oc = oracle_frame(oracle, sky, (shapes, tris, mats), rd, sd)
        t = tracer(T, sky, (shapes, tris, mats), rd, sd)
        trace_and_check(t, want, oc, GENERAL, (base, what))
        t.close()
