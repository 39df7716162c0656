"""X-ray area selection on the device (include/srt_abi.h "area selection, through"; csrc/area_through.hip): shape and triangle
coverage over each pixel ray's whole candidate set, the selection modes on top, the bounds and what the calls leave untouched.
Every expected value comes from tests/area_through_ref.py: the rays pick_rays returns, put through the CPU oracle's intersectors
(tests/multi_hit_ref.py) under the mask of tests/area_ref.py, compared with ==: everything here is an integer. The library is
never asked for a hit to make an expectation. Each scene's camera is shown to see through: some pixel has three candidates and
some shape counts on more pixels through than visibly (tests/test_area_through_host.py asserts the same without a device)."""
import ctypes

import numpy as np
import pytest

import area_ref as AR
import area_through_ref as XR
import cases as C
import gpu_harness as G
from area_through_cases import SCENES, arrays, frame_of, moved_mesh_scene
from gpu_harness import T  # noqa: F401 (the fixture)
from multi_hit_ref import words
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu
F = np.float32
DEVICE, MEDIAN = 1, 1  # SRT_BUILD_DEVICE, SRT_BUILD_ORDER_MEDIAN; also SRT_REFIT_DEVICE
ERR_INVALID = 1
ZERO = dict(area_pixels=0, hit_pixels=0, miss_pixels=0, distinct=0, target_pixels=0)


def handle(T, scn, accel="scan", rd=None, sky=None):
    sh, tr, ma = scn
    w, h = (8, 4) if rd is None else (int(rd["width"]), int(rd["height"]))
    t = T.Tracer(w, h)
    if sky is not None:
        t.set_skybox(sky)
    t.set_acceleration(0 if accel == "scan" else 1)
    if accel == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    if accel == "refit":
        t.set_acceleration_refit(DEVICE)
    if rd is not None:
        t.options = rd.copy()
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    return t


_lists = {}


def lists_of(T, oracle, name):
    """the reference's candidate list per pixel of the scene's frame, from pick_rays' rays, computed once and never changed"""
    if name not in _lists:
        scn, rd = (moved_mesh_scene(), frame_of("mesh_smooth")) if name == "mesh_moved" else (arrays(name), frame_of(name))
        w, h = int(rd["width"]), int(rd["height"])
        t = handle(T, scn, rd=rd)
        rays = t.pick_rays(XR.pixel_centres(w, h))
        t.close()
        _lists[name] = XR.candidate_lists(oracle, scn, rays)
    return _lists[name]


def check(t, lists, w, h, rect, lasso, n_shapes, what=""):
    counts, got = t.area_coverage(rect, lasso, through=True)
    want_counts, want = XR.coverage(lists, w, h, rect, lasso, n_shapes)
    print(f"{what} {rect}: got {counts.tolist()} {got}; want {want_counts.tolist()} {want}")
    assert got == want, (what, rect, got, want)
    assert np.array_equal(counts, want_counts), (what, rect, counts, want_counts)
    assert got["area_pixels"] == got["hit_pixels"] + got["miss_pixels"] and got["target_pixels"] == 0
    assert not t.last_area_id_pass()
    return counts, got


# ---- 1. pick rays ------------------------------------------------------------------------------------------------------------------
def test_pick_rays_are_the_rays_pick_through_casts(T):
    rd = frame_of("mesh_smooth")
    w, h = int(rd["width"]), int(rd["height"])
    t = handle(T, arrays("mesh_smooth"), "sah", rd)
    xy = np.concatenate([XR.pixel_centres(w, h)[:126], np.asarray([[3.25, 1.75], [0.0, 0.0], [w, h], [-2.5, 40.0]], F)])
    assert len(xy) == 130
    want_hits, want_counts = t.pick_through(xy, 4)
    rays = t.pick_rays(xy)
    assert (rays["tmax"] == np.inf).all()
    hits, counts = t.cast_rays_multi(rays, k=4, unit=True)
    assert np.array_equal(words(hits), words(want_hits)) and np.array_equal(counts, want_counts) and counts.max() >= 3
    whole = rays.view(np.uint32).reshape(len(xy), -1)
    for n in (0, 1, 63, 64, 65, 130):  # a call of n points returns the first n of them, each equal word for word
        part = t.pick_rays(xy[:n])
        assert part.shape == (n,)
        for q in range(n):
            assert np.array_equal(part[q:q + 1].view(np.uint32).ravel(), whole[q]), (n, q)
    lib, rdp = t.lib, R.as_records(rd, R.RENDER_DATA)
    out = np.zeros(1, R.RAY)
    assert lib.srt_pick_rays(t._h, None, T._ptr(xy), 1, T._ptr(out)) == ERR_INVALID
    assert lib.srt_pick_rays(t._h, T._ptr(rdp), None, 1, T._ptr(out)) == ERR_INVALID
    assert lib.srt_pick_rays(t._h, T._ptr(rdp), T._ptr(xy), 1, None) == ERR_INVALID and not out.view(np.uint32).any()
    assert lib.srt_pick_rays(t._h, None, None, 0, None) == 0
    t.close()


# ---- 2. shape coverage against the reference --------------------------------------------------------------------------------------
def sphere_rects(w, h):
    """widths 1, 63, 64, 65 and 130 and heights 1, 3, 4, 5 and 6 on the 130x6 frame: across wave and workgroup edges"""
    return [(0, 0, w, h), (7, 2, 8, 3), (3, 0, 66, 3), (66, 1, 130, 5), (0, 0, 64, 4), (33, 1, 98, 6), (1, 0, 66, 5), (-4, -2, 200, 9), (129, 5, 130, 6),
            (64, 0, 65, 6), (w, 0, w + 5, h), (5, 3, 5, 4)]


@pytest.mark.parametrize("name,accel", [(n, a) for n in SCENES for a in SCENES[n]["accels"]])
def test_shape_coverage_equals_the_reference(name, accel, T, oracle):
    rd = frame_of(name)
    w, h = int(rd["width"]), int(rd["height"])
    scn = arrays(name)
    n_shapes = len(scn[0])
    if accel == "refit":  # the scene moves under a hierarchy kept up on the device: the moved scene's reference
        t = handle(T, scn, "refit", rd)
        scn = moved_mesh_scene()
        t.update_scene(*scn)
        assert t.acceleration_refit_info()["models"] >= 1
        lists = lists_of(T, oracle, "mesh_moved")
        assert lists != lists_of(T, oracle, name)
    else:
        t = handle(T, scn, accel, rd)
        lists = lists_of(T, oracle, name)
    most, more = XR.sees_through(lists, w, h, n_shapes)
    assert most >= 3 and more, (name, most, more)
    rects = sphere_rects(w, h) if name == "spheres" else [(0, 0, w, h), (3, 2, w - 5, h - 3), (-2, 1, 7, h + 4), (w - 1, h - 1, w, h)]
    if name == "spheres":
        assert {r[2] - r[0] for r in rects} >= {1, 63, 64, 65, 130} and {r[3] - r[1] for r in rects} >= {1, 3, 4, 5, 6}
    for rect in rects:
        counts, s = check(t, lists, w, h, rect, None, n_shapes, what=(name, accel))
    full, s = t.area_coverage((0, 0, w, h), through=True)
    vis, vs = t.area_coverage((0, 0, w, h))
    assert (full >= vis).all() and (full > vis).any() and full.sum() > s["hit_pixels"] >= vs["hit_pixels"], (name, accel, full, vis)
    assert set(np.flatnonzero(full > vis).tolist()) & set(more)
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 3. lassos ----------------------------------------------------------------------------------------------------------------------
def wall_scene():
    """one plane that fills every frame looking down -z from the origin"""
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    sh = np.zeros(1, R.SHAPE)
    sh[0] = R.plane(0, (0, 0, -5.0), (0, 0, 1))
    return sh, R.box_triangles(), mats


@pytest.mark.parametrize("name", ["concave_U", "bow_tie", "zero_area", "far_outside", "zigzag_256", "diagonal_through_centres"])
def test_lasso_mask_is_the_host_mask(name, T, oracle):
    w, h = AR.W, AR.H
    lasso = AR.LASSOS[name]
    rd = R.render_data(w, h, 1, 1, camera_to_world=R.identity4(), time=1)
    wall = handle(T, wall_scene(), rd=rd)
    spheres = handle(T, arrays("spheres"), rd=frame_of("spheres", w, h))
    lists = None
    for rect in (AR.RECTS["inside"], (0, 0, w, h), AR.RECTS["over_right"]):
        m = T.area_mask(rect, lasso, w, h)
        assert np.array_equal(m, AR.mask(rect, lasso, w, h))
        counts, s = wall.area_coverage(rect, lasso, through=True)
        assert counts.tolist() == [int(m.sum())] and s == dict(area_pixels=int(m.sum()), hit_pixels=int(m.sum()), miss_pixels=0,
                                                                 distinct=int(m.any()), target_pixels=0), (name, rect, counts, s)
        assert spheres.area_coverage(rect, lasso, through=True)[1]["area_pixels"] == m.sum()
        if name in AR.EMPTY:
            assert not m.any()
        elif rect != AR.RECTS["over_right"]:
            assert 0 < m.sum() < (rect[2] - rect[0]) * (rect[3] - rect[1]), "the lasso cuts the rectangle"
    for y in (0, 4, 5, 17, 18, 31, 32, 36):  # row by row: rows above, across and below the lasso
        row = T.area_mask((0, y, w, y + 1), lasso, w, h)
        assert wall.area_coverage((0, y, w, y + 1), lasso, through=True)[0][0] == row.sum(), (name, y)
    if name == "bow_tie":  # ... and against the reference on a scene with several shapes and misses
        if "spheres_70" not in _lists:
            t = spheres
            _lists["spheres_70"] = XR.candidate_lists(oracle, arrays("spheres"), t.pick_rays(XR.pixel_centres(w, h)))
        for rect in (AR.RECTS["inside"], (0, 0, w, h)):
            counts, s = check(spheres, _lists["spheres_70"], w, h, rect, lasso, 7, what="bow_tie")
            assert s["distinct"] >= 2
    wall.close(), spheres.close()


# ---- 4. triangle coverage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_triangle_coverage_equals_the_reference(accel, T, oracle):
    rd = frame_of("mesh_smooth")
    w, h = int(rd["width"]), int(rd["height"])
    scn = arrays("mesh_smooth")
    lists = lists_of(T, oracle, "mesh_smooth")
    t = handle(T, scn, accel, rd)
    for s0 in (1, 2):
        n_tri = int(scn[0]["num_triangles"][s0])
        vis, _ = t.area_triangle_coverage(s0, n_tri, (0, 0, w, h))
        for rect, lasso in (((0, 0, w, h), None), ((2, 1, w - 3, h - 2), None), ((0, 0, w, h), [(1, 1), (w - 1, h - 2), (w - 1, 1), (1, h - 2)])):
            counts, s = t.area_triangle_coverage(s0, n_tri, rect, lasso, through=True)
            want_counts, want = XR.triangle_coverage(lists, w, h, s0, n_tri, rect, lasso)
            print(f"{accel} s0={s0} {rect}: got {s}, want {want}, sum {int(counts.sum())}")
            assert s == want and np.array_equal(counts, want_counts), (accel, s0, rect)
            assert not t.last_area_id_pass()
        # (the last area was the whole frame under a lasso; the statements below are about the whole frame)
        counts, s = t.area_triangle_coverage(s0, n_tri, (0, 0, w, h), through=True)
        assert s["target_pixels"] == s["hit_pixels"] > 0 and counts.sum() > s["target_pixels"], "target_pixels counts pixels, not crossings"
        assert ((vis == 0) & (counts > 0)).any(), "a face that is nowhere visible is counted through"
        assert (counts >= vis).all() and s["distinct"] == (counts > 0).sum()
    with pytest.raises(T.SrtError) as e:
        t.area_triangle_coverage(0, 16, (0, 0, w, h), through=True)  # the plane is no model
    assert e.value.code == ERR_INVALID
    with pytest.raises(T.SrtError) as e:
        t.area_triangle_coverage(1, n_tri - 1, (0, 0, w, h), through=True)  # one short
    assert e.value.code == ERR_INVALID
    with pytest.raises(T.SrtError) as e:
        t.area_triangle_coverage(3, n_tri, (0, 0, w, h), through=True)  # beyond the scene
    assert e.value.code == ERR_INVALID
    assert t.counters()["watchdog"] == 0
    t.close()


def test_a_sphere_is_no_model(T):
    t = handle(T, arrays("spheres"), rd=frame_of("spheres"))
    with pytest.raises(T.SrtError) as e:
        t.area_triangle_coverage(4, 16, (0, 0, 8, 4), through=True)
    assert e.value.code == ERR_INVALID
    t.close()


# ---- 5. directed cases --------------------------------------------------------------------------------------------------------------
def one_box():
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    sh = np.zeros(1, R.SHAPE)
    sh[0] = R.box_model(0, 0, (0.0, 0.0, 0.0))
    return sh, R.box_triangles(), mats


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_a_ray_through_a_shared_edge_counts_both_triangles_and_the_shape_once(accel, T, oracle):
    # a 1x1 frame: the pixel centre's ray is the view axis, (0, 0, 5) -> -z, through the +z face's diagonal (triangles 3 and 9)
    # and the -z face's (1 and 7), as tests/test_gpu_multi_hit.py shows for the same ray
    rd = R.render_data(1, 1, 1, 1, camera_to_world=R.camera_matrix((0.0, 0.0, 5.0), 0.0, 0.0), time=1)
    scn = one_box()
    t = handle(T, scn, accel, rd)
    rays = t.pick_rays([[0.5, 0.5]])
    assert np.array_equal(rays["origin"][0], F([0, 0, 5])) and np.array_equal(rays["direction"][0], F([0, 0, -1]))
    lists = XR.candidate_lists(oracle, scn, rays)
    assert sorted(c[2] for c in lists[0]) == [1, 3, 7, 9]
    counts, s = t.area_coverage((0, 0, 1, 1), through=True)
    assert counts.tolist() == [1] and s == dict(area_pixels=1, hit_pixels=1, miss_pixels=0, distinct=1, target_pixels=0)
    tri, s = t.area_triangle_coverage(0, 12, (0, 0, 1, 1), through=True)
    assert np.flatnonzero(tri).tolist() == [1, 3, 7, 9] and tri.max() == 1
    assert s == dict(area_pixels=1, hit_pixels=1, miss_pixels=0, distinct=4, target_pixels=1)
    t.close()


def test_camera_inside_a_sphere_counts_it_once_per_pixel(T, oracle):
    rd = frame_of("glass")
    w, h = int(rd["width"]), int(rd["height"])
    lists = lists_of(T, oracle, "glass")
    assert all(sum(1 for c in cl if c[1] == 1) == 1 for cl in lists)  # the exit alone
    t = handle(T, arrays("glass"), rd=rd)
    counts, s = t.area_coverage((0, 0, w, h), through=True)
    assert counts[1] == w * h and s["miss_pixels"] == 0
    t.close()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_small_frames(w, h, T, oracle):
    scn = arrays("spheres")
    rd = frame_of("spheres", w, h)
    t = handle(T, scn, rd=rd)
    lists = XR.candidate_lists(oracle, scn, t.pick_rays(XR.pixel_centres(w, h)))
    for rect in [(0, 0, w, h), (0, 0, 1, 1), (-3, -3, 9, 9), (w - 1, h - 1, w, h), (w, 0, w + 2, h)]:
        check(t, lists, w, h, rect, None, 7, what=(w, h))
    t.close()


def test_nothing_to_count(T):
    """a plane parallel to the one ray of a 1x1 frame, an empty scene, no scene at all, a NaN camera and an
    area wholly outside the frame: every pixel of the area is a miss, no count is written, no launch fails"""
    w, h = 9, 5
    rd = R.render_data(w, h, 1, 1, camera_to_world=R.camera_matrix((0.0, 0.0, 5.0), 0.0, 0.0), time=1)
    all_miss = dict(area_pixels=w * h, hit_pixels=0, miss_pixels=w * h, distinct=0, target_pixels=0)
    mats = np.zeros(1, R.MATERIAL)
    par = np.zeros(1, R.SHAPE)
    par[0] = R.plane(0, (0, -1.0, 0), (0, 1, 0))
    one = R.render_data(1, 1, 1, 1, camera_to_world=R.camera_matrix((0.0, 0.0, 5.0), 0.0, 0.0), time=1)
    t = handle(T, (par, R.box_triangles(), mats), rd=one)  # the one ray is (0, 0, -1): the plane's denominator is 0
    counts, s = t.area_coverage((0, 0, 1, 1), through=True)
    assert counts.tolist() == [0] and s == dict(area_pixels=1, hit_pixels=0, miss_pixels=1, distinct=0, target_pixels=0)
    t.close()
    t = T.Tracer(w, h)  # no scene yet
    t.options = rd
    counts, s = t.area_coverage((0, 0, w, h), through=True, n_shapes=0)
    assert len(counts) == 0 and s == all_miss
    t.scene_data = R.scene_data(0)  # an empty scene
    t.update_scene(*C.empty_scene())
    counts, s = t.area_coverage((0, 0, w, h), through=True, n_shapes=0)
    assert len(counts) == 0 and s == all_miss
    t.close()
    t = handle(T, arrays("spheres"), rd=rd)
    assert t.area_coverage((0, 0, w, h), through=True)[1]["hit_pixels"] > 0
    bad = rd.copy()
    bad["camera_to_world"][3, 0] = np.nan  # every ray's origin is NaN: refused on the device
    counts, s = t.area_coverage((0, 0, w, h), through=True, options=bad)
    assert not counts.any() and s == all_miss
    for rect in (AR.RECTS["outside"], AR.RECTS["outside_above"], AR.RECTS["empty_x"], AR.RECTS["empty_outside"]):
        counts, s = t.area_coverage(rect, through=True)
        assert not counts.any() and s == ZERO, rect
    assert t.counters()["watchdog"] == 0
    t.synchronize()
    t.close()


# ---- 6. capacities, state and errors --------------------------------------------------------------------------------------------------
def test_capacity_errors_and_the_device_form(T, oracle):
    import torch
    rd = frame_of("spheres")
    w, h = int(rd["width"]), int(rd["height"])
    lists = lists_of(T, oracle, "spheres")
    t = handle(T, arrays("spheres"), rd=rd)
    lib, p = t.lib, T._ptr
    rdp = R.as_records(rd, R.RENDER_DATA)
    a, _ = T.area_record((0, 0, w, h))
    counts, summary = np.full(7, 0xEEEEEEEE, np.uint32), np.full(8, 0xEEEEEEEE, np.uint32)
    assert lib.srt_area_coverage_through(t._h, p(rdp), p(a), None, p(counts), 6, p(summary)) == ERR_INVALID  # one short: nothing is launched
    assert lib.srt_area_coverage_through(t._h, None, p(a), None, p(counts), 7, p(summary)) == ERR_INVALID  # options is required
    assert lib.srt_area_coverage_through(t._h, p(rdp), None, None, p(counts), 7, p(summary)) == ERR_INVALID
    assert lib.srt_area_coverage_through(t._h, p(rdp), p(a), None, p(counts), 7, None) == ERR_INVALID
    assert lib.srt_area_coverage_through(None, p(rdp), p(a), None, p(counts), 7, p(summary)) == ERR_INVALID
    flagged, _ = T.area_record((0, 0, w, h))
    flagged["flags"] = 1
    assert lib.srt_area_coverage_through(t._h, p(rdp), p(flagged), None, p(counts), 7, p(summary)) == ERR_INVALID  # flags = 1 stays refused
    zero = rdp.copy()
    zero["width"] = 0
    assert lib.srt_area_coverage_through(t._h, p(zero), p(a), None, p(counts), 7, p(summary)) == ERR_INVALID
    assert lib.srt_area_triangle_coverage_through(t._h, None, p(a), None, 4, p(counts), 7, p(summary)) == ERR_INVALID
    n_sel = ctypes.c_size_t(0)
    assert lib.srt_select_area_through(t._h, None, p(a), None, 0, 1, ctypes.byref(n_sel)) == ERR_INVALID
    assert lib.srt_select_area_through(t._h, p(rdp), p(a), None, 4, 1, ctypes.byref(n_sel)) == ERR_INVALID
    assert (counts == 0xEEEEEEEE).all() and (summary == 0xEEEEEEEE).all() and len(t.read_selection()) == 0
    with pytest.raises(T.SrtError):
        t.read_id_pass()  # no through call makes ID planes
    with pytest.raises(T.SrtError) as e:
        t.area_coverage((0, 0, w, h), options=False, through=True)
    assert e.value.code == ERR_INVALID
    # the device form: all n words zeroed, n_shapes counted, nothing outside
    guard, n = 0x5EADBEEF, 11
    buf = torch.full((16 + n + 16 + 8 + 16,), guard, dtype=torch.int64, device="cuda").to(torch.int32)  # guards | counts | guards | summary | guards
    torch.cuda.synchronize()
    base = buf.data_ptr()
    for rect, lasso in [((0, 0, w, h), None), ((3, 0, 100, 5), [(4, 0), (90, 1), (70, 6), (10, 5)]), ((w + 2, 0, w + 9, h), None)]:
        t.area_coverage_device(base + 4 * 16, n, base + 4 * (16 + n + 16), rect, lasso, through=True)
        t.synchronize()
        host = buf.cpu().numpy().view(np.uint32)
        want_counts, want = XR.coverage(lists, w, h, rect, lasso, 7)
        assert np.array_equal(host[16:16 + 7], want_counts) and not host[16 + 7:16 + n].any(), rect
        s = host[16 + n + 16:16 + n + 16 + 8]
        assert s[:5].tolist() == [want[k] for k in R.AREA_SUMMARY.names[:5]] and not s[5:].any(), (rect, s, want)
        for lo, hi in ((0, 16), (16 + n, 16 + n + 16), (16 + n + 16 + 8, len(host))):
            assert (host[lo:hi] == guard).all(), (rect, lo)
    with pytest.raises(T.SrtError):
        t.area_coverage_device(base + 4 * 16, 6, base, (0, 0, w, h), through=True)
    with pytest.raises(T.SrtError):
        t.area_coverage_device(base + 4 * 16 + 2, n, base, (0, 0, w, h), through=True)  # not aligned
    with pytest.raises(T.SrtError):
        t.area_coverage_device(base + 4 * 16, n, base, (0, 0, w, h), options=False, through=True)
    t.close()


def frame(t, ticks=1):
    t.clear_canvas()
    return t.render(ticks).reshape(t.height, t.width, 4).copy()


def test_through_calls_leave_everything_else_alone(T, sky):
    w, h = AR.W, AR.H
    t = G.make(T, sky, arrays("spheres"), w, h, spp=1, time=777, denoise=dict(iterations=1))
    t.options = frame_of("spheres", w, h)
    t.set_kernel_timers(True)
    t.set_selection([4, 5], width=2.0)
    first = frame(t)
    assert t.last_resolve_selected() == (True, True)
    vis_before = t.area_coverage((5, 5, 60, 30), AR.LASSOS["bow_tie"])
    assert not t.last_area_id_pass()

    def state():
        ids = t.read_id_pass()
        return (t.counters(), t.read_canvas().view(np.uint32).copy(), t.read_argb().copy(), t.read_denoised().view(np.uint32).copy(), t.read_selection().copy(),
                ids["shape"], ids["triangle"], ids["material"], t.read_selection_alpha().copy(), t.last_trace_launches(), t.last_trace_class(),
                t.last_kernel_ms(), t.last_resolve_selected(), t.last_ray_query_ms())

    before = state()
    counts, s = t.area_coverage((5, 5, 60, 30), AR.LASSOS["bow_tie"], through=True)
    assert t.last_area_ms() > 0.0 and not t.last_area_id_pass() and s["distinct"] >= 2
    t.area_coverage((0, 0, w, h), through=True)
    after = state()
    assert before[0] == after[0] and after[0]["watchdog"] == 0 and before[9:] == after[9:]
    assert all(np.array_equal(a, b) for a, b in zip(before[1:9], after[1:9]))
    vis_after = t.area_coverage((5, 5, 60, 30), AR.LASSOS["bow_tie"])
    assert not t.last_area_id_pass()  # the planes were left as they were: no new ID pass
    assert np.array_equal(vis_before[0], vis_after[0]) and vis_before[1] == vis_after[1]
    assert np.array_equal(first, frame(t)) and t.last_resolve_selected() == (True, False)
    t.set_kernel_timers(False)
    t.area_coverage((0, 0, w, h), through=True)
    assert t.last_area_ms() == 0.0
    t.close()


# ---- 7. select_area(through=True) ----------------------------------------------------------------------------------------------------
def hidden_scene():
    """sphere 1 stands wholly behind sphere 0 as the camera at (0, 0, 5) sees them; sphere 2 beside them; no plane"""
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    sh = np.zeros(3, R.SHAPE)
    sh[0] = R.sphere(0, (0.0, 0.0, 0.0), 1.0)
    sh[1] = R.sphere(0, (0.0, 0.0, -3.0), 0.5)
    sh[2] = R.sphere(0, (2.0, 0.0, 0.0), 0.5)
    return sh, R.box_triangles(), mats


def test_select_area_through_modes_and_the_overlay(T, sky, oracle):
    w, h = 40, 24
    scn = hidden_scene()
    cam = R.camera_matrix((0.0, 0.0, 5.0), 0.0, 0.0)
    t = G.make(T, sky, scn, w, h, spp=1, time=777, cam=cam)
    t.options = R.render_data(w, h, 1, 2, fov_scale=0.5, camera_to_world=cam, time=777)
    off = frame(t)
    lists = XR.candidate_lists(oracle, scn, t.pick_rays(XR.pixel_centres(w, h)))
    rect = (2, 1, 30, 23)
    want_counts, _ = XR.coverage(lists, w, h, rect, None, 3)
    vis, _ = t.area_coverage(rect)
    assert vis[1] == 0 and want_counts[1] > 1 and want_counts[0] > want_counts[1], (vis, want_counts)  # hidden, and met through
    counts, _ = check(t, lists, w, h, rect, None, 3, what="hidden")
    current = [1, 2, 1000]
    for mode in (AR.ADD, AR.SUBTRACT, AR.TOGGLE, AR.REPLACE):
        t.set_selection(current, width=3.0)
        n = t.select_area(rect, mode=mode, through=True)
        want = AR.combine(current, want_counts, mode, 1)
        got = t.read_selection()
        assert n == len(want) and np.array_equal(got, want), (mode, got, want)
    assert 1 in got, "the hidden sphere is selected"
    c1 = int(want_counts[1])
    t.select_area(rect, min_pixels=c1, through=True)
    assert 1 in t.read_selection()
    t.select_area(rect, min_pixels=c1 + 1, through=True)
    assert 1 not in t.read_selection() and 0 in t.read_selection()
    t.select_area(rect, through=True)
    on = frame(t)
    assert t.last_resolve_selected()[0] and not np.array_equal(on, off)  # the overlay is enabled
    assert t.select_area((w + 1, 0, w + 5, h), through=True) == 0 and len(t.read_selection()) == 0  # an empty result: off
    assert np.array_equal(frame(t), off)
    assert t.select_area(rect, mode=AR.ADD, through=True) == len(np.flatnonzero(want_counts))  # ... and ADD starts from nothing
    t.close()


# ---- 8. the group ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_devices", [2, 3])
def test_group_forms_equal_the_single_handles(n_devices, T, sky):
    rd = frame_of("mesh_smooth")
    w, h = int(rd["width"]), int(rd["height"])
    sh, tr, ma = arrays("mesh_smooth")
    n_tri = int(sh["num_triangles"][1])
    lasso = [(1, 1), (w - 1, h - 2), (w - 1, 1), (1, h - 2)]
    single = handle(T, (sh, tr, ma), "sah", rd)
    want = [single.area_coverage((0, 0, w, h), through=True), single.area_coverage((1, 0, w - 2, h), lasso, through=True)]
    want_tri = single.area_triangle_coverage(1, n_tri, (0, 0, w, h), lasso, through=True)
    xy = XR.pixel_centres(w, h)[:65]
    want_rays = single.pick_rays(xy)
    single.close()
    g = T.TracerGroup(w, h, n_devices=n_devices, devices=[0] * n_devices, rows_per_block=1)
    g.set_skybox(sky)
    g.set_acceleration(1)
    g.options, g.scene_data = rd.copy(), R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    got = [g.area_coverage((0, 0, w, h), through=True), g.area_coverage((1, 0, w - 2, h), lasso, through=True)]
    for (a, sa), (b, sb) in zip(got, want):
        assert np.array_equal(a, b) and sa == sb
    got_tri = g.area_triangle_coverage(1, n_tri, (0, 0, w, h), lasso, through=True)
    assert np.array_equal(got_tri[0], want_tri[0]) and got_tri[1] == want_tri[1] and want_tri[1]["target_pixels"] > 0
    assert np.array_equal(g.pick_rays(xy).view(np.uint32), want_rays.view(np.uint32))
    n = g.select_area((0, 0, w, h), min_pixels=3, through=True)
    assert n == len(g.read_selection()) >= 2 and np.array_equal(g.read_selection(), AR.combine([], want[0][0], AR.REPLACE, 3))
    g.close()


# ---- 9. the headless route ------------------------------------------------------------------------------------------------------------
def test_headless_select_area_through_prints_the_python_paths_counts(T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    w, h = AR.W, AR.H
    prefix = str(tmp_path / "s")
    lasso = [(10, 2), (66, 6), (60, 35), (14, 30)]
    cmd = [exe, "--scene", "spheres", "--width", str(w), "--height", str(h), "--spp", "1", "--bounces", "2", "--frames", "1", "--select", "1:3",
           "--select-area", "5,3:64,33:add:40", "--lasso", ";".join(f"{x},{y}" for x, y in lasso), "--through", "--dump", prefix]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    t = T.Tracer(w, h)
    t.options = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    shapes = np.fromfile(prefix + ".shapes.bin", R.SHAPE)
    t.scene_data = np.fromfile(prefix + ".sd.bin", R.SCENE_DATA)[0]
    t.update_scene(shapes, np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    counts, s = t.area_coverage((5, 3, 64, 33), lasso, through=True)
    vis, _ = t.area_coverage((5, 3, 64, 33), lasso)
    assert (counts > vis).any() and s["distinct"] >= 2
    printed = {int(a): int(b) for a, b in re.findall(r"^shape (\d+) count (\d+)$", out, re.M)}
    assert printed == {int(i): int(c) for i, c in enumerate(counts) if c}, out
    sel = AR.combine([1], counts, AR.ADD, 40)
    assert f"area selection: {len(sel)} shape(s)\n" in out and f"selection: {len(sel)} shape(s)\n" in out, out
    t.close()
