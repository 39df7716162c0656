"""GPU (MI355X): the axis twins of the scene classes (DESIGN.md 5 "Axis planes"). A scene of class PPS whose three planes have
the normals +-e_y, +-e_x | +-e_z runs a kernel that folds each plane's two dot products into one subtraction and one component
read and divides without the compiler's scaling steps, behind one guard per EXTEND phase. None of it may change a bit.

* srt_selftest_plane_forms: whole waves run the twin's plane phase beside test_planes2, the rare operand nowhere, in one lane,
  in lane 0, in lane 63, in all lanes; tmin / best equal bit for bit and the fast branch is taken exactly where it is meant to be.
* Against the CPU oracle (canvas bits and counters) with srt_last_trace_plane_form asserted: the benchmark scene, hand-built
  in-pattern scenes, off-pattern neighbours (form 0), cameras on a plane / with -0 components / 1e20 away / NaN and inf, sample
  batches, a two-way row partition, and 200 hostile in-pattern scenes of a lane of this file's own.
* A direction exactly along an axis: the jitter never lands on the pixel centre exactly at these sizes (it would need
  random_float == 0.5 twice), so that case is driven through the self-test (dir = (0, 0, -1), two zero components: the guard's
  lower bound sends the wave to the reference's form).

CPU tests (no marker) hold the hostile lane to the cap of tests/test_fuzz_lanes.py and check each scene's pattern."""
import numpy as np
import pytest

import fuzz_scenes as FS
import test_gpu_camera_phase as CP
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
GENERAL, PPS, PPS_SPECULAR = 0, 1, 2
YXZ = 2 | (1 << 2) | (3 << 4)  # device_types.h SRT_AXES_PPS_YXZ: planes y, x | plane z
COUNTERS = CP.COUNTERS


def f2u(x):
    return np.asarray(x, F).view(np.uint32)


# ---- the self-test ------------------------------------------------------------------------------------------------------------------
def bench_planes():
    """the two staged plane blocks of the benchmark scene: {p, 0, n, 0} x 2 each, the fourth slot a filler"""
    shapes, _, _ = S.sphere_scene()
    blk = np.zeros(32, F)
    for i in range(3):
        assert int(shapes["type"][i]) == R.SHAPE_PLANE
        blk[8 * i:8 * i + 3] = shapes["plane_position"][i]
        blk[8 * i + 4:8 * i + 7] = shapes["plane_normal"][i]
    return blk


RARE = {  # name -> (org or None, dir or None, tmin or None): what replaces a lane's operands
    "numerator_zero": ((0.5, -1.0, 5.0), None, None),  # on the floor (y = -1)
    "numerator_neg_zero_side": ((-4.0, 0.5, 5.0), None, None),  # on the wall (x = -4)
    "org_neg_zero": ((-0.0, -1.0, -0.0), None, None),
    "org_nan": ((np.nan, 0.5, 5.0), None, None),
    "org_inf": ((0.5, np.inf, 5.0), None, None),
    "org_far": ((0.0, 0.5, 1e20), None, None),
    "dir_along_axis": (None, (0.0, 0.0, -1.0), None),
    "dir_neg_zero": (None, (-0.0, 0.6, -0.8), None),
    "dir_nan": (None, (np.nan, 0.6, -0.8), None),
    "dir_inf": (None, (0.1, np.inf, -0.8), None),
    "dir_tiny": (None, (1e-13, 0.6, -0.8), None),
    "dir_denormal": (None, (1e-45, 0.6, -0.8), None),
    "dir_huge": (None, (0.1, 0.6, 2e12), None),
}
PLACEMENTS = ["nowhere", "one_lane", "lane_0", "lane_63", "all_lanes"]


def selftest_words(rng, waves):
    n = waves * 64
    org = rng.uniform(-3, 3, (n, 3)) + np.array([0, 0.5, 4])
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    w = np.zeros((n, 8), np.uint32)
    w[:, 0:3], w[:, 3:6] = f2u(org), f2u(d)
    w[:, 6] = f2u(np.where(rng.rand(n) < 0.5, np.inf, rng.uniform(0.1, 20, n)))
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("what", [0, 1])
def test_selftest_plane_forms(what, T, sky):
    rng = np.random.RandomState(77 + what)
    names = sorted(RARE)
    words = selftest_words(rng, len(names) * len(PLACEMENTS))
    expect_fast = np.ones(len(names) * len(PLACEMENTS), bool)
    for i, name in enumerate(names):
        org, d, tm = RARE[name]
        if what == 1 and org is not None:
            continue  # a camera phase: the origin is the camera's for every lane (the cases below the loop)
        for j, place in enumerate(PLACEMENTS):
            wv = i * len(PLACEMENTS) + j
            lanes = {"nowhere": [], "one_lane": [int(rng.randint(1, 63))], "lane_0": [0], "lane_63": [63], "all_lanes": list(range(64))}[place]
            for ln in lanes:
                if org is not None: words[wv * 64 + ln, 0:3] = f2u(org)
                if d is not None: words[wv * 64 + ln, 3:6] = f2u(d)
            expect_fast[wv] = not lanes
    t = T.Tracer(8, 8)
    try:
        tame = 1 if what == 0 else 2  # the first cameras leave the numerators inside the box; the others are on a plane, NaN, far away
        cams = [(0.3, 0.5, 5.0), (-0.0, 0.5, -0.0), (0.5, -1.0, 5.0), (np.nan, 0.5, 5.0), (0.0, 0.5, 1e20)][:1 if what == 0 else 5]
        for k, cam in enumerate(cams):
            new, ref, fast, bad = t.selftest_plane_forms(what, bench_planes(), cam, words)
            print("what", what, "camera", cam, "fast waves", int(fast.sum()), "of", len(fast), "mismatching words", bad)
            assert bad == 0 and np.array_equal(new, ref), (what, cam, np.flatnonzero((new != ref).any(axis=1))[:8])
            if k < tame:
                assert np.array_equal(fast.astype(bool), expect_fast), (what, cam, np.flatnonzero(fast.astype(bool) != expect_fast))
            else:
                assert not fast.any(), (what, cam)  # a hostile camera origin: no wave may take the fast branch
            if k < tame:
                assert (ref[:, 1] != 0xFFFFFFFF).any()  # the planes are hit by somebody (a NaN origin hits nothing)
    finally:
        t.close()


# ---- against the oracle ---------------------------------------------------------------------------------------------------------------
def with_planes(normals=None, positions=None, order=None):
    shapes, tris, mats = CP.base_scene()
    if order is not None:
        shapes[:3] = shapes[:3][list(order)]
    for i, n in (normals or {}).items():
        shapes["plane_normal"][i] = n
    for i, p in (positions or {}).items():
        shapes["plane_position"][i] = p
    return shapes, tris, mats


def run_case(T, sky, oracle, scn, rd, cls, form, what, sd=None, expect_fail=None):
    want, oc = CP.oracle_frame(oracle, sky, scn, rd, sd)
    t = CP.tracer(T, sky, scn, rd, sd)
    try:
        d = CP.trace_and_check(t, want, oc, cls, what)
        assert t.last_trace_plane_form() == form, (what, t.last_trace_plane_form(), form)
        print(what, "axis phases", d["axis_phases"], "failed the guard", d["axis_failed"])
        if form:
            assert d["axis_phases"] > 0 and d["axis_failed"] <= d["axis_phases"], (what, d)
            if expect_fail is True: assert d["axis_failed"] > 0, (what, d)
            if expect_fail is False: assert d["axis_failed"] * 20 <= d["axis_phases"], (what, d)
    finally:
        t.close()


IN_PATTERN = {
    "benchmark": lambda: CP.base_scene(),
    "all_negative_normals": lambda: with_planes({0: (0, -1, 0), 1: (-1, 0, 0), 2: (0, 0, -1)}),
    "zeros_written_as_neg_zero": lambda: with_planes({0: (-0.0, 1, -0.0), 1: (1, -0.0, -0.0), 2: (-0.0, -0.0, 1)}),
    "moved_planes": lambda: with_planes({1: (-1, 0, 0)}, {0: (7.0, -1.5, -3.0), 1: (-3.25, 100.0, 0.0), 2: (1e10, -2e10, -5.0)}),
}
OFF_PATTERN = {
    "tilted_1e-30": lambda: with_planes({0: (0, 1, 1e-30)}),
    "length_2": lambda: with_planes({0: (0, 2, 0)}),
    "two_planes_swapped": lambda: with_planes(order=(1, 0, 2)),
    "position_not_finite": lambda: with_planes(positions={2: (np.inf, 0.0, -6.0)}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(IN_PATTERN))
def test_in_pattern_scenes_run_the_twin(name, T, sky, oracle):
    for w, h, spp in ((64, 32, 16), (96, 64, 64)) if name == "benchmark" else ((64, 32, 64),):
        run_case(T, sky, oracle, IN_PATTERN[name](), CP.options(w, h, spp), PPS, YXZ, (name, w, h, spp), expect_fail=False)


@pytest.mark.gpu
def test_specular_class_has_its_twin(T, sky, oracle):
    shapes, tris, mats = CP.base_scene()
    mats["specular"][0] = 0.5
    run_case(T, sky, oracle, (shapes, tris, mats), CP.options(64, 32, 32), PPS_SPECULAR, YXZ, "specular")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OFF_PATTERN))
def test_off_pattern_neighbours_run_the_class_kernel(name, T, sky, oracle):
    run_case(T, sky, oracle, OFF_PATTERN[name](), CP.options(64, 32, 32), PPS, 0, name)


AXIS_CAMERAS = {
    # exactly axis-aligned basis (camera_matrix with zero angles), on planes, with -0 components, far away, not finite
    "on_floor": (R.camera_matrix((1.0, -1.0, 5.0), 0.0, 0.0), True),
    "on_wall": (R.camera_matrix((-4.0, 0.5, 5.0), 0.0, 0.0), True),
    "neg_zero_origin": (CP.edited(CP.edited(R.camera_matrix((0.0, 0.5, 5.0), 0.0, 0.0), 3, 0, -0.0), 3, 1, -0.0), None),
    "far_away": (R.camera_matrix((0.0, 0.5, 1e20), 0.0, 0.0), True),
    "nan_origin": (CP.edited(S.default_camera(), 3, 0, np.nan), True),
    "inf_origin": (CP.edited(S.default_camera(), 3, 1, np.inf), True),
    "inf_rotation": (CP.edited(S.default_camera(), 0, 0, np.inf), True),
    "axis_aligned_basis": (R.camera_matrix((0.0, 0.5, 5.0), 0.0, 0.0), False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(AXIS_CAMERAS))
def test_cameras_at_the_guard(name, T, sky, oracle):
    cam, expect_fail = AXIS_CAMERAS[name]
    for scene in ("benchmark", "all_negative_normals"):
        run_case(T, sky, oracle, IN_PATTERN[scene](), CP.options(64, 32, 32, cam), PPS, YXZ, (name, scene), expect_fail=expect_fail)


@pytest.mark.gpu
def test_sample_batches(T, sky, oracle):
    w, h, spp = 64, 32, 50
    scn, rd = CP.base_scene(), CP.options(64, 32, 50)
    want, oc = CP.oracle_frame(oracle, sky, scn, rd)
    t = CP.tracer(T, sky, scn, rd)
    t.set_radiance_budget(w * h * 12 * 17)
    CP.trace_and_check(t, want, oc, PPS, "three batches")
    assert t.last_trace_plane_form() == YXZ and t.last_trace_launches()[0] >= 3
    t.close()


@pytest.mark.gpu
def test_two_way_row_partition(T, sky, oracle):
    w, h, spp = 64, 32, 32
    scn, rd = CP.base_scene(), CP.options(w, h, spp)
    want, oc = CP.oracle_frame(oracle, sky, scn, rd)
    total = dict.fromkeys(("paths", "rays", "sky"), 0)
    for rank in range(2):
        t = CP.tracer(T, sky, scn, rd)
        t.set_partition(rank, 2, 8)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        assert t.last_trace_class() == PPS and t.last_trace_plane_form() == YXZ
        part, c = t.read_canvas(), t.counters()
        assert t.owned_rows > 0 and c["watchdog"] == 0
        for r in range(t.owned_rows):
            assert bits_equal(part[r], want[T.global_row(h, rank, 2, 8, r)]), (rank, r)
        for k in total:
            total[k] += c[k]
        t.close()
    assert total == {k: oc[k] for k in total}, (total, oc)


# ---- 200 hostile in-pattern scenes ------------------------------------------------------------------------------------------------------
HOSTILE_N, HOSTILE_SEED = 200, 212121
_hostile, _hostile_want = [], []


def axis_lane_scene(rng, it):
    """a hostile scene of class PPS / PPS_SPECULAR (tests/fuzz_scenes.py class_scene: hostile radii, materials and cameras) whose
    planes are axis planes in the pattern y, x | z: signs and zero signs random, positions now and then huge, on the camera or
    with a -0; the camera now and then exactly on a plane"""
    cls = PPS if it % 2 == 0 else PPS_SPECULAR
    shapes, tris, mats, cam, rd, sd = FS.class_scene(rng, cls, True, 16, 16)
    for i, k in enumerate((1, 0, 2)):
        n = np.where(rng.rand(3) < 0.5, 0.0, -0.0)
        n[k] = rng.choice([1.0, -1.0])
        shapes["plane_normal"][i] = n
        p = shapes["plane_position"][i].copy()
        r = rng.rand()
        if r < 0.10: p[k] = cam[3, k]  # the camera on the plane: num = +-0
        elif r < 0.15: p[k] = rng.choice([1e12, -1e16, 2.0 ** 50, 1e-30, -0.0])
        elif r < 0.20: p[(k + 1) % 3] = rng.choice([1e25, 2.0 ** 100, -0.0])
        shapes["plane_position"][i] = p
    if rng.rand() < 0.1:
        cam[3, int(rng.randint(3))] = rng.choice([-0.0, 0.0])
        rd["camera_to_world"] = cam
    rd["num_samples"] = int(rng.choice([1, 5, 64, 70]))
    return cls, shapes, tris, mats, rd, sd


def hostile_scenes():
    if not _hostile:
        rng = np.random.RandomState(HOSTILE_SEED)
        _hostile.extend(axis_lane_scene(rng, it) for it in range(HOSTILE_N))
    return _hostile


def hostile_want(oracle, sky):
    if not _hostile_want:
        _hostile_want.extend(CP.oracle_frame(oracle, sky, (s, t, m), rd, sd) for _, s, t, m, rd, sd in hostile_scenes())
    return _hostile_want


def test_hostile_lane_is_in_pattern_and_shows_something(sky, oracle):
    """CPU, the oracle alone: every scene is of its class by the restatement and its planes get the codes y, x, z from the library's
    predicate; at most a quarter are mostly NaN or sky"""
    from simple_raytracer_amd import tracer as TR
    blank = 0
    for (cls, shapes, tris, mats, rd, sd), (want, oc) in zip(hostile_scenes(), hostile_want(oracle, sky)):
        assert FS.expected_class(shapes, mats, rd) == cls
        assert [TR.plane_axis_code_host(shapes["plane_normal"][i], shapes["plane_position"][i]) for i in range(3)] == [2, 1, 3]
        empty_sd = sd.copy()
        empty_sd["num_shapes"] = 0
        with np.errstate(all="ignore"):
            nothing = oracle.render(rd, empty_sd, shapes[:0], tris, mats, sky, nthreads=4)
        nan = np.isnan(want[..., :3]).any(axis=-1)
        only_sky = (want.view(np.uint32) == nothing.view(np.uint32)).all(axis=-1)
        blank += int((nan | only_sky).mean() > 0.5)
    print(f"{blank} of {HOSTILE_N} hostile axis scenes mostly NaN or sky")
    assert blank <= HOSTILE_N // 4, blank


@pytest.mark.gpu
def test_hostile_in_pattern_scenes(T, sky, oracle):
    t = T.Tracer(16, 16)
    t.set_skybox(sky)
    bad, failed, phases = [], 0, 0
    try:
        for it, ((cls, shapes, tris, mats, rd, sd), (want, oc)) in enumerate(zip(hostile_scenes(), hostile_want(oracle, sky))):
            t.options, t.scene_data = rd, sd
            t.update_scene(shapes, tris, mats)
            t.clear_canvas()
            t.reset_counters()
            t.trace()
            got, c, d = t.read_canvas(), t.counters(), t.debug_counters()
            ctr = {k: (c[k], oc[k]) for k in COUNTERS if c[k] != oc[k]}
            failed, phases = failed + d["axis_failed"], phases + d["axis_phases"]
            if t.last_trace_class() != cls or t.last_trace_plane_form() != YXZ or not bits_equal(got, want) or ctr or c["watchdog"] != 0:
                bad.append((it, t.last_trace_class(), t.last_trace_plane_form(), FS.differing_pixels(got, want), ctr, c["watchdog"]))
    finally:
        t.close()
    print("axis phases", phases, "failed the guard", failed)
    assert not bad, bad
    assert 0 < failed < phases  # both branches ran
