"""Multi-hit ray queries on the device (include/srt_abi.h "multi-hit ray queries"; csrc/multi_hit.hip, csrc/device_multihit.h):
every record's t, shape and triangle word for word against the ordered candidate lists of tests/multi_hit_ref.py -- built from
the CPU oracle's intersectors, never from the library -- under the array scan, the host's SAH tree and the device's median
tree; the other fields against the cast where a record coincides with a cast record, and for records behind the first against
a cast of the same ray in a scene reduced to that one primitive; directed tie and limit cases, SRT_RAYS_COUNT_ALL, the directed
walk cases, hostile rays, state, errors, the group forms and the headless tool."""
import numpy as np
import pytest

import bvh_walk_cases as W
import cases as C
import multi_hit_ref as M
from gpu_harness import T  # noqa: F401 (the fixture)
from multi_hit_ref import MISS, words
from ray_query_cases import ACCELS, CAMERAS, FH, FW, frame_rd, jitter_xy, o_hits, primary, scene
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
SRT_ERR_INVALID = 1
KS = (1, 2, 3, 8)
NS_RAYS = (1, 63, 64, 65, 130)
SCENES = {"spheres": ACCELS["spheres"], "boxes": ("scan", "sah", "median"), "mesh_smooth": ACCELS["mesh_smooth"], "glass": ("scan",)}
GLASS_CAMERAS = (S.default_camera(), R.camera_matrix((4.0, 1.5, -5.0), -3.0, -0.1))


DEVICE, MEDIAN = 1, 1  # SRT_BUILD_DEVICE, SRT_BUILD_ORDER_MEDIAN; also SRT_REFIT_DEVICE


def handle(T, scn, accel="scan", sky=None, w=FW, h=FH, refit=False):
    sh, tr, ma = scene(scn) if isinstance(scn, str) else scn
    t = T.Tracer(w, h)
    if sky is not None:
        t.set_skybox(sky)
    t.set_acceleration(0 if accel == "scan" else 1)
    if accel == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    if refit:
        t.set_acceleration_refit(DEVICE)
    t.options = frame_rd(S.default_camera())
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    return t


def arrays(name):
    return C.glass_scene() if name == "glass" else scene(name)


_rays, _lists = {}, {}


def rays_of(oracle, name):
    """130 primary rays of the scene's two cameras (64 each, then camera 0's first two again): origins, unit directions"""
    if name not in _rays:
        o, d = [], []
        for k in (0, 1):
            if name == "glass":
                cam = GLASS_CAMERAS[k]
                sh, tr, ma = arrays(name)
                ids, sm = np.repeat(np.arange(FW * FH), 2), np.tile(np.arange(2), FW * FH)
                ph = o_hits(oracle, frame_rd(cam), sh, tr, ma, ids, sm)
            else:
                cam, ph = CAMERAS[name][k], primary(oracle, name, k)[2]
            o.append(np.tile(cam[3, :3], (len(ph["dir"]), 1))), d.append(ph["dir"])
        o, d = np.concatenate(o).astype(F), np.concatenate(d).astype(F)
        _rays[name] = (np.concatenate([o, o[:2]]), np.concatenate([d, d[:2]]))
    return _rays[name]


def lists_of(oracle, name):
    """the reference's candidate lists of rays_of(name), computed once and never changed"""
    if name not in _lists:
        o, d = rays_of(oracle, name)
        _lists[name] = M.Reference(oracle, *arrays(name)).lists(o, d)
    return _lists[name]


def check_fields_behind(T, scn, o, d, hits, tri_materials=None, limit=16):
    """normal, material and flags of up to `limit` records behind the first: a cast of the same ray in a scene reduced to that
    one primitive (a sphere, a plane, or the one triangle of its model) gives the same t, normal, flags and material"""
    sh, tr, ma = scn
    picks = [(q, j) for q in range(hits.shape[0]) for j in range(1, hits.shape[1]) if hits[q, j]["flags"] & R.HIT_HIT]
    picks = picks[::max(1, len(picks) // limit)][:limit]
    probe = T.Tracer(FW, FH)
    probe.set_acceleration(0)
    for q, j in picks:
        h = hits[q, j]
        one = sh[[int(h["shape"])]].copy()
        if h["triangle"] != R.HIT_NONE:
            one["triangle_index"] += h["triangle"]
            one["num_triangles"] = 1
        probe.scene_data = R.scene_data(1)
        probe.update_scene(one, tr, ma)
        c = probe.cast_rays(o[q], d[q], unit=True)[0]
        assert F(c["t"]).view(np.uint32) == F(h["t"]).view(np.uint32), (q, j, "t")
        assert np.array_equal(c["normal"].view(np.uint32), h["normal"].view(np.uint32)) and c["flags"] == h["flags"], (q, j, "normal / flags")
        if tri_materials is None:
            assert c["material"] == h["material"], (q, j, "material")
    probe.close()
    return len(picks)


# ---- 1. oracle primary rays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [(n, a) for n in SCENES for a in SCENES[n]])
def test_records_equal_the_oracle_lists(name, accel, T, oracle):
    o, d = rays_of(oracle, name)
    lists = lists_of(oracle, name)
    assert max(len(c) for c in lists) >= 3, [len(c) for c in lists]
    t = handle(T, arrays(name), accel)
    cast = t.cast_rays(o, d, unit=True)
    for k in KS:
        for n in NS_RAYS:
            hits, counts = t.cast_rays_multi(o[:n], d[:n], k, unit=True)
            M.check(hits, counts, lists[:n], k, what=(name, accel, k, n))
            # record 0 coincides with the cast's record: every word is the cast's. Where it does not, the oracle's list (checked above)
            # decides: the cast tests a model's box against its shrinking closest distance, this query against the caller's tmax
            same = (hits[:, 0]["t"].view(np.uint32) == cast[:n]["t"].view(np.uint32)) & (hits[:, 0]["shape"] == cast[:n]["shape"]) & \
                   (hits[:, 0]["triangle"] == cast[:n]["triangle"])
            if not same.all():
                print(f"{name}/{accel} k={k} n={n}: record 0 differs from the cast on rays {np.flatnonzero(~same).tolist()} (the model box's limit)")
            assert np.array_equal(words(hits[:, 0][same]), words(cast[:n][same])), (name, accel, k, n)
    hits, _ = t.cast_rays_multi(o, d, 8, unit=True)
    assert check_fields_behind(T, arrays(name), o, d, hits) >= 4
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 2. directed cases ---------------------------------------------------------------------------------------------------------
def stack_scene():
    """ten spheres and ten parallel planes along the ray (0,0,0) -> -z, stored in DECREASING distance: every insertion is at
    the front, and there are more candidates than the largest k"""
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    sh = np.zeros(20, R.SHAPE)
    for i in range(10):
        sh[i] = R.sphere(0, (0, 0, -(60.0 - 3.0 * i)), 0.5)
        sh[10 + i] = R.plane(0, (0, 0, -(30.0 - 3.0 * i)), (0, 0, 1))
    return sh, R.box_triangles(), mats


def one_box(position=(0.0, 0.0, 0.0), material=0):
    mats = np.zeros(2, R.MATERIAL)
    mats[0], mats[1] = R.material((0.8, 0.8, 0.8)), R.material((0.2, 0.9, 0.2))
    sh = np.zeros(1, R.SHAPE)
    sh[0] = R.box_model(material, 0, position)
    return sh, R.box_triangles(), mats


def test_more_candidates_than_k_all_inserted_at_the_front(T, oracle):
    scn = stack_scene()
    o, d = np.zeros((1, 3), F), np.asarray([[0, 0, -1]], F)
    lists = M.Reference(oracle, *scn).lists(o, d)
    assert [c[1] for c in lists[0]] == list(range(19, 9, -1)) + list(range(9, -1, -1))
    t = handle(T, scn)
    for k in (1, 2, 4, 8):
        hits, counts = t.cast_rays_multi(o, d, k, unit=True)
        M.check(hits, counts, lists, k, what=k)
        assert counts[0] == k and (hits[0]["flags"] == (R.HIT_HIT | R.HIT_FRONT)).all()
    # tmax exactly the third hit's t: strict, two records
    hits, counts = t.cast_rays_multi(o, d, 8, tmax=lists[0][2][0], unit=True)
    M.check(hits, counts, [lists[0][:2]], 8, what="tmax = third t")
    assert counts[0] == 2
    t.close()


def test_identical_spheres_tie_goes_to_array_order(T, oracle):
    sh, tr, ma = S.sphere_scene()
    two = np.zeros(3, R.SHAPE)
    two[0] = two[2] = R.sphere(0, (0.5, 0.25, -4.0), 1.0)
    two[1] = R.sphere(-1, (0.5, 0.25, -9.0), 1.5)  # behind them, without a material
    o, d = np.zeros((1, 3), F), np.asarray([[0.125, 0.0625, -1.0]], F)
    d = (d / np.sqrt((d.astype(np.float64) ** 2).sum())).astype(F)
    lists = M.Reference(oracle, two, tr, ma).lists(o, d)
    assert [c[1] for c in lists[0]] == [0, 2, 1] and lists[0][0][0] == lists[0][1][0]
    t = handle(T, (two, tr, ma))
    hits, counts = t.cast_rays_multi(o, d, 3, unit=True)
    M.check(hits, counts, lists, 3)
    assert np.array_equal(words(hits[0, 0])[0, [0, 3, 4, 5, 6, 7]], words(hits[0, 1])[0, [0, 3, 4, 5, 6, 7]])
    # a shape without a material behind one with a material: reported, material -1
    assert hits[0, 2]["material"] == -1 and hits[0, 2]["flags"] & R.HIT_HIT and hits[0, 0]["material"] == 0
    assert check_fields_behind(T, (two, tr, ma), o, d, hits) == 2
    t.close()


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_shared_diagonal_gives_two_records_lower_triangle_first(accel, T, oracle):
    scn = one_box()
    # the +z face is triangles 3 (5, 0, 4) and 9 (5, 1, 0) of R.box_triangles: they share the diagonal x == y
    o = np.asarray([[0.0, 0.0, 5.0], [0.5, 0.5, 5.0], [-0.25, -0.25, 5.0]], F)
    d = np.tile(np.asarray([0, 0, -1], F), (3, 1))
    lists = M.Reference(oracle, *scn).lists(o, d)
    for cl in lists:
        assert len(cl) >= 3 and cl[0][0] == cl[1][0] and (cl[0][2], cl[1][2]) == (3, 9), cl
    assert len(lists[0]) == 4 and lists[0][2][0] == lists[0][3][0] and (lists[0][2][2], lists[0][3][2]) == (1, 7)  # the back face's other diagonal too
    t = handle(T, scn, accel)
    for k in (1, 2, 3, 4, 8):
        hits, counts = t.cast_rays_multi(o, d, k, unit=True)
        M.check(hits, counts, lists, k, what=(accel, k))
    t.close()


def test_origin_inside_a_sphere_gives_its_exit(T, oracle):
    sh, tr, ma = C.glass_scene()
    o, d = np.asarray([[0, 0.5, 5.0]], F), np.asarray([[0, 0, -1]], F)  # inside shape 1
    lists = M.Reference(oracle, sh, tr, ma).lists(o, d)
    assert lists[0][0][1] == 1 and sum(1 for c in lists[0] if c[1] == 1) == 1
    t = handle(T, (sh, tr, ma))
    hits, counts = t.cast_rays_multi(o, d, 8, unit=True)
    M.check(hits, counts, lists, 8)
    assert hits[0, 0]["flags"] == R.HIT_HIT  # a back face: the normal was turned
    assert abs(float(hits[0, 0]["t"]) - 1.2) < 1e-5
    t.close()


@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_per_triangle_material_on_a_record_behind_the_first(accel, T, oracle):
    scn = one_box()
    o, d = np.asarray([[0.3, 0.2, 5.0]], F), np.asarray([[0, 0, -1]], F)
    lists = M.Reference(oracle, *scn).lists(o, d)
    assert len(lists[0]) == 2
    t = handle(T, scn, accel)
    before, _ = t.cast_rays_multi(o, d, 2, unit=True)
    tm = np.full(12, -1, np.int32)
    tm[lists[0][1][2]] = 1
    t.set_triangle_materials(tm)
    after, counts = t.cast_rays_multi(o, d, 2, unit=True)
    M.check(after, counts, lists, 2)
    assert (before[0]["material"] == 0).all() and after[0, 0]["material"] == 0 and after[0, 1]["material"] == 1
    for f in ("t", "shape", "triangle", "normal", "flags"):
        assert np.array_equal(after[f], before[f]), f
    t.close()


# ---- 3. SRT_RAYS_COUNT_ALL -----------------------------------------------------------------------------------------------------
def test_count_all_counts_the_whole_set(T, oracle):
    scn = stack_scene()
    o, d = np.zeros((1, 3), F), np.asarray([[0, 0, -1]], F)
    lists = M.Reference(oracle, *scn).lists(o, d)
    t = handle(T, scn)
    for k in (1, 2, 8):
        plain, _ = t.cast_rays_multi(o, d, k, unit=True)
        hits, counts = t.cast_rays_multi(o, d, k, unit=True, count_all=True)
        M.check(hits, counts, lists, k, count_all=True)
        assert counts[0] == 20 and np.array_equal(words(hits), words(plain))
    t.close()
    for name, accel in (("mesh_smooth", "scan"), ("mesh_smooth", "sah"), ("boxes", "median"), ("spheres", "scan")):
        o, d = rays_of(oracle, name)
        t = handle(T, arrays(name), accel)
        plain, _ = t.cast_rays_multi(o, d, 2, unit=True)
        hits, counts = t.cast_rays_multi(o, d, 2, unit=True, count_all=True)
        M.check(hits, counts, lists_of(oracle, name), 2, count_all=True, what=(name, accel))
        assert np.array_equal(words(hits), words(plain)) and (counts > 2).any(), (name, accel)
        t.close()


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_crossing_parity_tells_inside_from_outside(accel, T, oracle):
    scn = one_box((0.25, -0.5, 0.125))
    rng = np.random.default_rng(11)
    d = rng.normal(size=(64, 3))
    d = (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(F)  # generic directions: off every edge and diagonal
    centre = np.asarray((0.25, -0.5, 0.125), F)
    inside = (centre + rng.uniform(-0.9, 0.9, size=(64, 3))).astype(F)
    outside = (centre + np.where(rng.uniform(size=(64, 3)) < 0.5, -1.0, 1.0) * rng.uniform(1.2, 3.0, size=(64, 3))).astype(F)
    ref = M.Reference(oracle, *scn)
    t = handle(T, scn, accel)
    for o, odd in ((inside, 1), (outside, 0)):
        lists = ref.lists(o, d)
        hits, counts = t.cast_rays_multi(o, d, 4, unit=True, count_all=True)
        M.check(hits, counts, lists, 4, count_all=True, what=(accel, odd))
        assert (counts % 2 == odd).all(), (accel, odd, counts)
    assert (counts == 2).any() and (counts == 0).any()
    t.close()


# ---- 4. walk edge cases --------------------------------------------------------------------------------------------------------
# exact-plane rays (into the box, away from it, and along the plane with a +0 and a -0 component across it) and axis-parallel rays
WALK_FAMILIES = ("on_plane_in", "on_plane_out", "on_plane_along", "axis_parallel")
_walk = {}


def walk_cases(oracle, mesh, kind, fam):
    """per record of the family on the planes of the tree `kind` (bvh_walk_cases.oracle_subset's four per mesh and tree): origins
    and unit directions of every (pixel, sample) of its frame, and their candidate lists, computed once"""
    if (mesh, kind, fam) not in _walk:
        sc = W.scene(mesh)
        scn = (sc["shapes"], sc["tris"], sc["mats"])
        ref, out = M.Reference(oracle, *scn), []
        for rec in W.oracle_subset(mesh, kind, fam):
            rd = W.render_data(rec)
            ns = int(rd["num_samples"])
            ids, sm = np.repeat(np.arange(W.W * W.H), ns), np.tile(np.arange(ns), W.W * W.H)
            ph = o_hits(oracle, rd, *scn, ids, sm)
            o = np.tile(rd["camera_to_world"][3, :3], (len(ids), 1)).astype(F)
            out.append((rec["name"], o, ph["dir"], ref.lists(o, ph["dir"])))
        _walk[(mesh, kind, fam)] = out
    return _walk[(mesh, kind, fam)]


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
@pytest.mark.parametrize("mesh", W.MESH_NAMES)
def test_walk_edge_cases_at_k4(mesh, accel, T, oracle):
    sc = W.scene(mesh)
    t = handle(T, (sc["shapes"], sc["tris"], sc["mats"]), accel, w=W.W, h=W.H)
    on_model = {fam: 0 for fam in WALK_FAMILIES}
    for kind in (W.TREES if accel == "scan" else (accel,)):  # a tree walks the cases made on its own planes, the scan both trees'
        for fam in WALK_FAMILIES:
            cases = walk_cases(oracle, mesh, kind, fam)
            assert len(cases) >= 3, (mesh, kind, fam)
            for name, o, d, lists in cases:
                hits, counts = t.cast_rays_multi(o, d, 4, unit=True)
                M.check(hits, counts, lists, 4, what=(name, accel))
                on_model[fam] += int(((hits["shape"] == 0) & (hits["flags"] & R.HIT_HIT != 0)).any())
    print(f"{mesh}/{accel}: records with a hit on the model, per family: {on_model}")
    assert on_model["on_plane_in"] >= 2 and on_model["axis_parallel"] >= 2, on_model  # (the cast test's non-vacuous families)
    t.close()


# ---- 5. hostile rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_hostile_rays_get_the_invalid_record_in_every_slot(accel, T, oracle):
    o, d = rays_of(oracle, "mesh_smooth")
    lists = lists_of(oracle, "mesh_smooth")
    q = next(i for i, c in enumerate(lists) if len(c) >= 2)
    t = handle(T, "mesh_smooth", accel)
    for unit in (True, False):
        rays = R.rays(o[q], np.tile(d[q], (9, 1)))
        rays["origin"][0, 1] = np.nan
        rays["direction"][1, 2] = np.inf
        rays["direction"][2] = 0.0
        rays["tmax"][3] = np.nan
        rays["origin"][5, 0] = -np.inf
        rays["direction"][6, 0] = np.nan
        bad = [0, 1, 2, 3, 5, 6]
        if not unit:
            rays["direction"][7] = (1e-30, 0.0, 0.0)  # its squared length underflows
            rays["direction"][8] = (1e30, 1e30, 0.0)  # ... overflows
            bad += [7, 8]
        for k in (1, 3, 8):
            hits, counts = t.cast_rays_multi(rays, k=k, unit=unit)
            want = MISS.copy()
            want["flags"] = R.HIT_INVALID_RAY
            assert np.array_equal(words(hits[bad]), np.tile(words(want), (len(bad) * k, 1))), (unit, k)
            assert not counts[bad].any()
            if unit:
                M.check(hits[[4, 7, 8]], counts[[4, 7, 8]], [lists[q]] * 3, k, what="the valid rays among them")
            else:
                assert hits[4, 0]["shape"] == lists[q][0][1] and counts[4] == min(k, len(lists[q]))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 6. state, errors, device form, group, headless ------------------------------------------------------------------------------
def test_a_query_leaves_the_frame_alone(T, sky, oracle):
    o, d = rays_of(oracle, "mesh_smooth")
    t = handle(T, "mesh_smooth", "sah", sky=sky)
    t.options = frame_rd(CAMERAS["mesh_smooth"][0])
    t.set_kernel_timers(True)
    t.set_denoise(feature_samples=1)
    t.set_noise_meter(min_samples=1, check_every=1)
    t.clear_canvas()
    t.trace()
    t.meter_noise()
    assert t.read_noise()["dispatches"] == 1

    def state():
        dn, ex, noise = t.read_denoise_inputs(), t.read_exposure(), dict(t.read_noise())
        planes = [dn["normal_depth"], dn["albedo_hits"], dn["moments"], ex["hist"], noise.pop("hist")]
        assert t.poll_noise() is not None  # (the metering's copy has landed: nothing is in flight across the query)
        return (t.read_canvas().view(np.uint32).copy(), [np.ascontiguousarray(a).view(np.uint32).copy() for a in planes], noise, dn["T"], dn["P"],
                ex["log2_exposure"], ex["metered"], t.last_meter_ran(), t.counters(), t.debug_counters(), t.last_trace_launches(),
                t.last_trace_kernel_ms(), t.last_kernel_ms(), t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured())

    before = state()
    hits, counts = t.cast_rays_multi(o[:64], d[:64], 4, unit=True)
    picked, _ = t.pick_through([[3.5, 1.5]], 3)
    assert t.last_ray_query_ms() > 0.0
    after = state()
    assert np.array_equal(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[1], after[1])) and before[2:] == after[2:]
    assert counts.any() and picked.shape == (1, 3)
    t.close()


def test_every_ray_misses_before_a_scene_is_set(T):
    t = T.Tracer(FW, FH)
    hits, counts = t.cast_rays_multi((0, 0, 5), [(0, 0, -1), (0, -1, 0), (1, 2, 3)], 3)
    assert np.array_equal(words(hits), np.tile(words(MISS), (9, 1))) and not counts.any()
    hits, counts = t.pick_through([[4.0, 2.0]], 2)
    assert np.array_equal(words(hits), np.tile(words(MISS), (2, 1))) and not counts.any()
    t.close()


def test_a_query_sees_the_updated_and_the_refitted_scene(T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    o, d = rays_of(oracle, "mesh_smooth")
    o, d = o[:64], d[:64]
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    lists = M.Reference(oracle, moved, tr, ma).lists(o, d)
    assert lists != lists_of(oracle, "mesh_smooth")[:64]
    for accel, refit in (("scan", False), ("sah", True), ("median", True)):
        t = handle(T, "mesh_smooth", accel, refit=refit)
        t.update_scene(moved, tr, ma)
        if refit:
            assert t.acceleration_refit_info()["models"] >= 1
        hits, counts = t.cast_rays_multi(o, d, 3, unit=True)
        M.check(hits, counts, lists, 3, what=(accel, "after the move"))
        t.close()


def test_counts_and_argument_errors_on_a_handle(T):
    t = handle(T, "spheres")
    hits, counts = t.cast_rays_multi(np.zeros((0, 3), F), np.zeros((0, 3), F), 2)
    assert hits.shape == (0, 2) and len(counts) == 0 and t.pick_through(np.zeros((0, 2), F), 2)[0].shape == (0, 2)
    rays, hits, counts = np.zeros(1, R.RAY), np.zeros((1, 8), R.RAY_HIT), np.zeros(1, np.uint32)
    rays["origin"], rays["direction"], rays["tmax"] = (0.0, 0.5, 5.0), (0, 0, -1), np.inf  # the default camera's view axis: it meets shape 4
    rd, xy = R.as_records(t.options, R.RENDER_DATA), np.zeros((1, 2), F)
    p, lib, h = T._ptr, t.lib, t._h
    assert lib.srt_cast_rays_multi(h, None, 0, 1, 0, None, None) == 0 and lib.srt_cast_rays_multi_device(h, None, 0, 8, 3, None, None) == 0
    assert lib.srt_pick_through(h, None, None, 0, 1, None, None) == 0
    for k in (0, 9):
        assert lib.srt_cast_rays_multi(h, p(rays), 1, k, 0, p(hits), p(counts)) == SRT_ERR_INVALID
        assert lib.srt_cast_rays_multi(h, None, 0, k, 0, None, None) == SRT_ERR_INVALID
        assert lib.srt_pick_through(h, p(rd), p(xy), 1, k, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_multi(h, p(rays), 1, 2, 4, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_multi(h, None, 1, 2, 0, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_multi(h, p(rays), 1, 2, 0, None, p(counts)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_multi_device(h, None, 1, 2, 0, None, None) == SRT_ERR_INVALID
    assert lib.srt_pick_through(h, None, p(xy), 1, 2, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_pick_through(h, p(rd), None, 1, 2, p(hits), p(counts)) == SRT_ERR_INVALID
    assert not hits.view(np.uint32).any() and not counts.any()
    assert lib.srt_cast_rays_multi(h, p(rays), 1, 2, 0, p(hits), None) == 0  # counts are optional
    assert hits[0, 0]["flags"] & R.HIT_HIT
    t.close()


@pytest.mark.parametrize("n", [1, 65])
def test_device_form_tails_and_alignment(n, T, oracle):
    import torch
    o, d = rays_of(oracle, "mesh_smooth")
    rays = R.rays(o[:n], d[:n])
    k = 3
    t = handle(T, "mesh_smooth", "sah")
    want, want_counts = t.cast_rays_multi(rays, k=k, unit=True)
    dev = torch.device("cuda", 0)
    rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
    pattern = np.int32(0x5A5A5A5A)
    hits_dev = torch.full((n * k + 64, 8), int(pattern), dtype=torch.int32, device=dev)
    counts_dev = torch.full((n + 64,), int(pattern), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.cast_rays_multi_device(rays_dev.data_ptr(), n, k, hits_dev.data_ptr(), counts_dev.data_ptr(), unit=True)
    t.synchronize()
    got, got_counts = hits_dev.cpu().numpy(), counts_dev.cpu().numpy()
    assert np.array_equal(got[:n * k].view(np.uint32), words(want)) and (got[n * k:] == pattern).all()
    assert np.array_equal(got_counts[:n].view(np.uint32), want_counts) and (got_counts[n:] == pattern).all()
    lib, h = t.lib, t._h
    for rp, hp, cp in ((rays_dev.data_ptr() + 4, hits_dev.data_ptr(), 0), (rays_dev.data_ptr(), hits_dev.data_ptr() + 8, 0),
                       (rays_dev.data_ptr(), hits_dev.data_ptr(), counts_dev.data_ptr() + 2)):
        assert lib.srt_cast_rays_multi_device(h, rp, n, k, 1, hp, cp or None) == SRT_ERR_INVALID
    t.synchronize()
    assert np.array_equal(hits_dev.cpu().numpy(), got)
    t.close()


def test_group_forms_and_pick_through_equal_the_single_handles(T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    cam = CAMERAS["mesh_smooth"][1]
    ids, sm, ph = primary(oracle, "mesh_smooth", 1)
    rd = frame_rd(cam)
    xy = jitter_xy(oracle, rd, ids, sm)
    t = handle(T, "mesh_smooth", "sah")
    g = T.TracerGroup(FW, FH, n_devices=2, devices=[0, 0], rows_per_block=1)
    g.set_acceleration(1)
    g.scene_data = R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    a, ac = t.cast_rays_multi(cam[3, :3], ph["dir"], 3, unit=True)
    b, bc = g.cast_rays_multi(cam[3, :3], ph["dir"], 3, unit=True)
    assert np.array_equal(words(a), words(b)) and np.array_equal(ac, bc)
    pa, pac = t.pick_through(xy, 3, options=rd)
    pb, pbc = g.pick_through(xy, 3, options=rd)
    # the picked rays are the samples' primary rays bit for bit (srt_pick's kernel), so pick_through equals the cast of them
    assert np.array_equal(words(pa), words(a)) and np.array_equal(pac, ac)
    assert np.array_equal(words(pb), words(pa)) and np.array_equal(pbc, pac)
    assert np.array_equal(words(pa[:, 0]), words(t.pick(xy, options=rd)))
    g.close(), t.close()


HEADLESS_PICKS = {
    "spheres": [((32.0, 24.0), 3), ((10.5, 40.5), 8), ((50.25, 12.75), 1), ((32.5, 1.5), 2)],
    # the tool's mesh scene without model files: a floor and the box model at (2.5, -0.2, -3), which the default camera sees around
    # pixel (39.5, 26) of a 64x48 frame, three pixels to either side; then a floor point and a miss
    "meshes": [((39.5, 26.5), 4), ((38.25, 25.0), 8), ((41.0, 27.5), 2), ((24.5, 26.5), 8), ((32.0, 24.0), 4)],
}


@pytest.mark.parametrize("scn", ["spheres", "meshes"])
def test_headless_pick_through_prints_pythons_records(scn, T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    w, h = 64, 48
    picks = HEADLESS_PICKS[scn]
    prefix = str(tmp_path / "p")
    cmd = [exe, "--scene", scn, "--width", str(w), "--height", str(h), "--spp", "1", "--bounces", "1", "--frames", "1", "--dump", prefix]
    for (x, y), k in picks:
        cmd += ["--pick-through", f"{x},{y}:{k}"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("pick-through ")]
    sh, tr, ma = (np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    rd = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    cam = rd["camera_to_world"].astype(np.float64)
    t = handle(T, (sh, tr, ma), w=w, h=h)
    num = r"(\S+)"
    line_re = re.compile(rf"^pick-through {num},{num}: shape (\d+) triangle (-?\d+) material (-?\d+) t {num} position {num} {num} {num} normal {num} {num} {num}$")
    at, seen, on_model = 0, 0, 0
    for (x, y), k in picks:
        want, count = t.pick_through([(x, y)], k, options=rd)
        # the point's ray as the tool forms it on the host for the printed position (the formulas of srt_pick's header text), in double
        sx, sy = (2.0 * (x / w) - 1.0) * float(rd["aspect_ratio"]) * float(rd["fov_scale"]), (1.0 - 2.0 * (y / h)) * float(rd["fov_scale"])
        v = cam[0, :3] * sx + cam[1, :3] * sy - cam[2, :3]
        d, o = v / np.sqrt((v * v).sum()), cam[3, :3]
        for j in range(int(count[0])):
            rec = want[0, j]
            m = line_re.match(lines[at])
            assert m, lines[at]
            assert (float(m.group(1)), float(m.group(2))) == (x, y), lines[at]
            assert int(m.group(3)) == rec["shape"] and int(m.group(5)) == rec["material"], lines[at]
            assert int(m.group(4)) == (-1 if rec["triangle"] == R.HIT_NONE else int(rec["triangle"])), lines[at]
            assert F(m.group(6)) == rec["t"], lines[at]  # %.9g round-trips a float32
            assert np.array_equal(np.asarray([F(m.group(g)) for g in (10, 11, 12)]).view(np.uint32), rec["normal"].view(np.uint32)), lines[at]
            # the position is origin + direction * t in float32 with a direction normalised on the host: a few roundings of 2^-24
            # relative in the direction, scaled by t, and one of the sum -- 8 * 2^-23 of the magnitudes involved bounds them
            pos = np.asarray([float(m.group(g)) for g in (7, 8, 9)])
            assert np.all(np.abs(pos - (o + d * float(rec["t"]))) <= 8 * 2.0 ** -23 * (np.abs(o).max() + float(rec["t"]))), lines[at]
            on_model += int(rec["triangle"] != R.HIT_NONE)
            at += 1
            seen += 1
        assert lines[at] == f"pick-through {x:g},{y:g}: {int(count[0])} hit(s)", lines[at]
        at += 1
    assert at == len(lines) and seen >= 4, out
    assert on_model >= 2 or scn == "spheres", out  # the mesh scene's points print model records, triangle column and all
    t.close()
