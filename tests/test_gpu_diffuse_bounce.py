"""GPU (MI355X): the diffuse waves of the NO_SPEC scene classes (DESIGN.md 5 "Diffuse waves"). A SHADE phase whose shading lanes
all have a plain diffuse material (metallic and transmittance threshold 0) and whose operands pass one voted guard takes
random_dir as the new direction: no material draws, no reflect3, no mix3. None of it may change a bit.

* srt_selftest_diffuse_bounce: whole waves run the wave form beside the per-lane form with each kind of offending operand
  nowhere, in one random lane, in lane 0, in lane 63, in all lanes: 0 mismatching words, and the short form is taken exactly
  when no lane offends. The short form's outputs are checked against numpy, too.
* Against the CPU oracle (canvas bits and counters), with the two counters read (debug_counters()["diffuse_short"],
  ["diffuse_failed"]; "shade_phases" is counted by these kernels). A SHADE phase whose lanes are all on their last bounce runs no
  bounce at all; with all its lanes plain diffuse it counts as short, which is what makes `short == shade_phases` exact for the
  all-diffuse scene. A wave that ran the short form on a lane that must not have it (NaN smoothness, a huge normal) would leave a
  finite direction where the oracle has a NaN one: the canvas bits and the NaN-pixel counter see that.

CPU tests (no marker) hold every scene to two conditions with the oracle alone, so that no scene can hide a failure: hand-built
scenes show at least half of their pixels finite and bounce (rays > paths); of the 200 hostile scenes at most a quarter are mostly
NaN or sky (the cap of tests/test_fuzz_lanes.py). The camera with a NaN component is the one exception, stated at SHOWS_NOTHING_BY_CONSTRUCTION."""
import numpy as np
import pytest

import fuzz_scenes as FS
import test_gpu_camera_phase as CP
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
GENERAL, PPS, PPS_SPECULAR, SSS, PPP = 0, 1, 2, 3, 4
COUNTERS = CP.COUNTERS


def f2u(x):
    return np.asarray(x, F).view(np.uint32)


# ---- the self-test ------------------------------------------------------------------------------------------------------------------
# name -> (first word, the words that replace a lane's): {0..2 random_dir, 3..5 dir, 6..8 nrm, 9 metallic, 10 transmittance, 11 smoothness}
OFFENDERS = {
    "glass_lane": (10, np.array([0xFFFFFFFF], np.uint32)),
    "glass_lane_threshold_1": (10, np.array([1], np.uint32)),
    "metal_lane": (9, np.array([0x80000000], np.uint32)),
    "random_dir_plus_zero": (1, f2u([0.0])),
    "random_dir_minus_zero": (2, f2u([-0.0])),
    "smoothness_nan": (11, f2u([np.nan])),
    "smoothness_inf": (11, f2u([np.inf])),
    "smoothness_huge": (11, f2u([1e30])),
    "normal_huge": (6, f2u([0.0, 1e20, 0.0])),
    "normal_2^21": (7, f2u([2.0 ** 21])),
    "dir_inf": (3, f2u([np.inf])),
    "dir_nan": (5, f2u([np.nan])),
}
PLACEMENTS = ["nowhere", "one_lane", "lane_0", "lane_63", "all_lanes"]
REPEATS = 5  # 12 kinds x 5 placements x 5 = 300 waves


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def selftest_words(rng, waves):
    n = waves * 64
    w = np.zeros((n, 20), np.uint32)
    w[:, 0:3], w[:, 3:6], w[:, 6:9] = f2u(unit(rng, n)), f2u(unit(rng, n)), f2u(unit(rng, n))
    w[:, 11] = f2u(rng.choice([0.0, 1.0, 0.3, 0.9], n))
    w[:, 12:15], w[:, 15:18] = f2u(rng.uniform(0, 1, (n, 3))), f2u(rng.uniform(0, 1, (n, 3)))
    w[:, 18] = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    assert (w[:, 0:3].view(F) != 0).all()
    return w


@pytest.mark.gpu
def test_selftest_diffuse_bounce(T, sky):
    rng = np.random.RandomState(2201)
    names = sorted(OFFENDERS)
    waves = len(names) * len(PLACEMENTS) * REPEATS
    words = selftest_words(rng, waves)
    expect_fast = np.ones(waves, bool)
    wv = 0
    for name in names:
        at, val = OFFENDERS[name]
        for place in PLACEMENTS:
            for _ in range(REPEATS):
                lanes = {"nowhere": [], "one_lane": [int(rng.randint(1, 63))], "lane_0": [0], "lane_63": [63], "all_lanes": list(range(64))}[place]
                for ln in lanes:
                    words[wv * 64 + ln, at:at + len(val)] = val
                expect_fast[wv] = not lanes
                wv += 1
    t = T.Tracer(8, 8)
    try:
        new, ref, fast, bad = t.selftest_diffuse_bounce(words)
    finally:
        t.close()
    fast = fast.astype(bool)
    print("waves", waves, "short form", int(fast.sum()), "mismatching words", bad, "lanes that drew transparent", int(ref[:, 7].sum()))
    assert bad == 0 and np.array_equal(new, ref), np.flatnonzero((new != ref).any(axis=1))[:8]
    assert np.array_equal(fast, expect_fast), np.flatnonzero(fast != expect_fast)
    assert ref[:, 7].sum() > 0  # the glass lanes were drawn transparent by the per-lane form
    # the short form's own outputs: random_dir, mask * colour, the generator three steps on
    ln = np.repeat(fast, 64)
    assert ln.sum() >= 64 * len(names) * REPEATS
    assert np.array_equal(new[ln, 0:3], words[ln, 0:3])
    assert np.array_equal(new[ln, 3:6], f2u(words[ln, 12:15].view(F) * words[ln, 15:18].view(F)))
    seed = words[ln, 18].astype(np.uint64)
    for _ in range(3):
        seed = (seed * 747796405 + 2891336453) & 0xFFFFFFFF
    assert np.array_equal(new[ln, 6], seed.astype(np.uint32)) and not new[ln, 7].any()


# ---- against the oracle ---------------------------------------------------------------------------------------------------------------
def bench_scene(edit=None):
    shapes, tris, mats = CP.base_scene()
    if edit:
        edit(shapes, mats)
    return shapes, tris, mats


def all_diffuse(shapes, mats):
    mats["metallic"], mats["transmittance"] = 0.0, 0.0


def all_glass_or_metal(shapes, mats):
    for i in range(len(mats)):
        mats[i]["metallic" if i % 2 else "transmittance"] = 1.0
        mats[i]["smoothness"] = 0.7


def nan_smoothness_floor(shapes, mats):
    all_diffuse(shapes, mats)
    mats["smoothness"][int(shapes["material"][6])] = np.nan  # the small sphere on the floor


def box_scene(normal_edit):
    """six planes, class PPP (general planes 2 | 2 | 2): a room around the default camera; one stored normal edited"""
    mats = S.sphere_scene_materials().copy()
    mats["metallic"], mats["transmittance"] = 0.0, 0.0
    mats["smoothness"] = 0.5
    planes = [((0, -1, 0), (0, 1, 0)), ((-4, 0, 0), (1, 0, 0)), ((0, 0, -6), (0, 0, 1)), ((4, 0, 0), (-1, 0, 0)), ((0, 4, 0), (0, -1, 0)), ((0, 0, 8), (0, 0, -1))]
    shapes = FS.stack([R.plane(i, p, n) for i, (p, n) in enumerate(planes)], R.SHAPE)
    shapes["plane_normal"][5] = normal_edit  # the wall behind the camera: only bounced rays reach it
    return shapes, FS.NO_TRIS, mats


def cam_edit(row, col, v):
    return CP.edited(S.default_camera(), row, col, v)


# name -> (scene, options, class, what the counters must show)
CASES = {
    "benchmark_64x48x16": (lambda: bench_scene(), lambda: CP.options(64, 48, 16), PPS, "some"),
    "benchmark_48x32x64": (lambda: bench_scene(), lambda: CP.options(48, 32, 64), PPS, "some"),
    "benchmark_fewer_than_64_items": (lambda: bench_scene(), lambda: CP.options(1, 3, 16), PPS, None),
    "all_diffuse": (lambda: bench_scene(all_diffuse), lambda: CP.options(64, 48, 16), PPS, "all"),
    "all_diffuse_fewer_than_64_items": (lambda: bench_scene(all_diffuse), lambda: CP.options(1, 3, 16), PPS, "all"),
    "all_glass_or_metal": (lambda: bench_scene(all_glass_or_metal), lambda: CP.options(64, 48, 16), PPS, "none"),
    "nan_smoothness_diffuse": (lambda: bench_scene(nan_smoothness_floor), lambda: CP.options(64, 48, 16), PPS, "all_diffuse_some_failed"),
    "general_planes_normal_1e20": (lambda: box_scene((0, 0, -1e20)), lambda: CP.options(64, 48, 16, bounces=4), PPP, "all_diffuse_some_failed"),
    "general_planes_normal_zero": (lambda: box_scene((0, 0, 0)), lambda: CP.options(64, 48, 16, bounces=4), PPP, "all_diffuse"),
    "camera_1e20_away": (lambda: bench_scene(), lambda: CP.options(64, 48, 16, R.camera_matrix((0.0, 0.5, 1e20), 0.0, 0.0)), PPS, None),
    "camera_nan_component": (lambda: bench_scene(), lambda: CP.options(64, 48, 16, cam_edit(3, 0, np.nan)), PPS, None),
    "twelve_spheres": (lambda: sss_scene(), lambda: CP.options(64, 48, 16), SSS, "some"),
}
# A NaN anywhere in the camera's matrix reaches every ray's direction (the position column times w = 0 is added to it), so every
# pixel of that frame is NaN in the oracle and nobody bounces: the case runs (bits and counters), the two conditions cannot hold.
SHOWS_NOTHING_BY_CONSTRUCTION = {"camera_nan_component"}


def sss_scene():
    rng = np.random.RandomState(5)
    mats = S.sphere_scene_materials().copy()
    items = [R.sphere(int(i % 7), rng.uniform(-2.5, 2.5, 3) + np.array([0, 0.5, -1.0]), rng.uniform(0.4, 1.0)) for i in range(11)]
    items.append(R.sphere(0, (0.0, 0.5, 0.0), 9.0))  # encloses the others and the camera
    return FS.stack(items, R.SHAPE), FS.NO_TRIS, mats


_want = {}


def want_of(name, oracle, sky):
    if name not in _want:
        scene, opts, _, _ = CASES[name]
        _want[name] = (scene(), opts(), *CP.oracle_frame(oracle, sky, scene(), opts()))
    return _want[name]


def check_diffuse_counters(d, expect, what):
    print(what, "shade phases", d["shade_phases"], "short", d["diffuse_short"], "all diffuse but failed the guard", d["diffuse_failed"])
    assert d["diffuse_short"] + d["diffuse_failed"] <= d["shade_phases"], (what, d)
    if expect is not None:
        assert d["shade_phases"] > 0, (what, d)  # (a camera with a NaN component hits nothing: no SHADE phase at all)
    if expect == "some":
        assert 0 < d["diffuse_short"] < d["shade_phases"], (what, d)
    elif expect == "all":
        assert d["diffuse_short"] == d["shade_phases"] and d["diffuse_failed"] == 0, (what, d)
    elif expect == "none":
        assert d["diffuse_short"] == 0 and d["diffuse_failed"] == 0, (what, d)
    elif expect == "all_diffuse":
        assert d["diffuse_short"] + d["diffuse_failed"] == d["shade_phases"] and d["diffuse_short"] > 0, (what, d)
    elif expect == "all_diffuse_some_failed":
        assert d["diffuse_short"] + d["diffuse_failed"] == d["shade_phases"] and d["diffuse_failed"] > 0, (what, d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_scenes_show_something(name, sky, oracle):
    """CPU, the oracle alone: at least half of the pixels finite, and somebody bounced"""
    scn, rd, want, oc = want_of(name, oracle, sky)
    assert FS.expected_class(scn[0], scn[2], rd) == CASES[name][2]
    finite = np.isfinite(want[..., :3]).all(axis=-1).mean()
    print(name, "finite pixels", finite, "paths", oc["paths"], "rays", oc["rays"])
    if name in SHOWS_NOTHING_BY_CONSTRUCTION:
        return
    assert finite >= 0.5 and oc["rays"] > oc["paths"], (name, finite, oc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scenes_against_the_oracle(name, T, sky, oracle):
    scn, rd, want, oc = want_of(name, oracle, sky)
    t = CP.tracer(T, sky, scn, rd)
    try:
        d = CP.trace_and_check(t, want, oc, CASES[name][2], name)
        check_diffuse_counters(d, CASES[name][3], name)
    finally:
        t.close()


@pytest.mark.gpu
def test_sample_batches(T, sky, oracle):
    """a radiance budget that forces sample batches (two or more launches; the sum is carried across them)"""
    w, h, spp = 64, 48, 16
    scn, rd, want, oc = want_of("benchmark_64x48x16", oracle, sky)
    t = CP.tracer(T, sky, scn, rd)
    try:
        t.set_radiance_budget(w * h * 12 * 15)  # not all 16 samples at once: the launcher splits the frame into batches
        d = CP.trace_and_check(t, want, oc, PPS, "two batches")
        assert t.last_trace_launches()[0] >= 2
        check_diffuse_counters(d, "some", "two batches")
    finally:
        t.close()


@pytest.mark.gpu
def test_rank_1_of_3_row_partition(T, sky, oracle):
    w, h, spp = 64, 48, 16
    scn, rd, want, oc = want_of("benchmark_64x48x16", oracle, sky)
    t = CP.tracer(T, sky, scn, rd)
    try:
        t.set_partition(1, 3, 8)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        assert t.last_trace_class() == PPS
        part, c, d = t.read_canvas(), t.counters(), t.debug_counters()
        assert t.owned_rows > 0 and c["watchdog"] == 0
        for r in range(t.owned_rows):
            assert bits_equal(part[r], want[T.global_row(h, 1, 3, 8, r)]), r
        check_diffuse_counters(d, "some", "rank 1 of 3")
    finally:
        t.close()


def specular_scene():
    shapes, tris, mats = CP.base_scene()
    mats["specular"][0] = 0.5
    return shapes, tris, mats


def two_sphere_scene():
    mats = S.sphere_scene_materials().copy()
    return FS.stack([R.sphere(0, (0.0, 0.5, 0.0), 9.0), R.sphere(1, (0.0, 0.0, -1.0), 1.0)], R.SHAPE), FS.NO_TRIS, mats


@pytest.mark.gpu
@pytest.mark.parametrize("name,cls", [("general", GENERAL), ("specular_class", PPS_SPECULAR)])
def test_other_kernels_count_nothing(name, cls, T, sky, oracle):
    scn = two_sphere_scene() if cls == GENERAL else specular_scene()
    rd = CP.options(64, 48, 16)
    want, oc = CP.oracle_frame(oracle, sky, scn, rd)
    assert oc["rays"] > oc["paths"]
    t = CP.tracer(T, sky, scn, rd)
    try:
        d = CP.trace_and_check(t, want, oc, cls, name)
        assert d["diffuse_short"] == 0 and d["diffuse_failed"] == 0, (name, d)
    finally:
        t.close()


# ---- 200 hostile scenes of the NO_SPEC classes ------------------------------------------------------------------------------------------
HOSTILE_N, HOSTILE_SEED = 200, 220022
NO_SPEC_CLASSES = (PPS, PPS, SSS, PPP)  # (the benchmark's layout twice as often)
_hostile, _hostile_want = [], []


def hostile_scenes():
    if not _hostile:
        rng = np.random.RandomState(HOSTILE_SEED)
        for it in range(HOSTILE_N):
            cls = NO_SPEC_CLASSES[it % len(NO_SPEC_CLASSES)]
            shapes, tris, mats, cam, rd, sd = FS.class_scene(rng, cls, True, 16, 16)
            rd["num_samples"] = int(rng.choice([1, 5, 16, 70]))
            _hostile.append((cls, shapes, tris, mats, rd, sd))
    return _hostile


def hostile_want(oracle, sky):
    if not _hostile_want:
        _hostile_want.extend(CP.oracle_frame(oracle, sky, (s, t, m), rd, sd) for _, s, t, m, rd, sd in hostile_scenes())
    return _hostile_want


def test_hostile_scenes_are_in_class_and_show_something(sky, oracle):
    """CPU, the oracle alone: every scene is of its class by the restatement; at most a quarter are mostly NaN or sky"""
    blank = 0
    for (cls, shapes, tris, mats, rd, sd), (want, oc) in zip(hostile_scenes(), hostile_want(oracle, sky)):
        assert FS.expected_class(shapes, mats, rd) == cls
        empty_sd = sd.copy()
        empty_sd["num_shapes"] = 0
        with np.errstate(all="ignore"):
            nothing = oracle.render(rd, empty_sd, shapes[:0], tris, mats, sky, nthreads=4)
        nan = np.isnan(want[..., :3]).any(axis=-1)
        only_sky = (want.view(np.uint32) == nothing.view(np.uint32)).all(axis=-1)
        blank += int((nan | only_sky).mean() > 0.5)
    print(f"{blank} of {HOSTILE_N} hostile NO_SPEC scenes mostly NaN or sky")
    assert blank <= HOSTILE_N // 4, blank


@pytest.mark.gpu
def test_hostile_scenes(T, sky, oracle):
    t = T.Tracer(16, 16)
    t.set_skybox(sky)
    bad, short, failed, phases = [], 0, 0, 0
    try:
        for it, ((cls, shapes, tris, mats, rd, sd), (want, oc)) in enumerate(zip(hostile_scenes(), hostile_want(oracle, sky))):
            t.options, t.scene_data = rd, sd
            t.update_scene(shapes, tris, mats)
            t.clear_canvas()
            t.reset_counters()
            t.trace()
            got, c, d = t.read_canvas(), t.counters(), t.debug_counters()
            ctr = {k: (c[k], oc[k]) for k in COUNTERS if c[k] != oc[k]}
            short, failed, phases = short + d["diffuse_short"], failed + d["diffuse_failed"], phases + d["shade_phases"]
            if t.last_trace_class() != cls or not bits_equal(got, want) or ctr or c["watchdog"] != 0:
                bad.append((it, t.last_trace_class(), cls, FS.differing_pixels(got, want), ctr, c["watchdog"]))
    finally:
        t.close()
    print("shade phases", phases, "short", short, "all diffuse but failed the guard", failed)
    assert not bad, bad
    assert 0 < short < phases and failed > 0  # every branch ran
