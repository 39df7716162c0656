"""Area selection on the device (include/srt_abi.h "area selection"; csrc/area.hip): marquee and lasso coverage, triangle coverage,
the selection modes, the bounds and what the calls leave untouched. Every expected value is the numpy restatement (tests/area_ref.py)
applied to the ID planes read from the device with read_id_pass, compared with ==: everything here is an integer.

Frames are 70x37: no multiple of 64, 32, 8 or 4. Scenes and cameras are the selection tests': the sphere scene under CAM_A (fov 0.25:
sphere 4 in the middle, 3 and 5 cut by the borders) and CAM_C (fov 0.35), the smooth-mesh scene from close by. Every case asserts on
the device's planes that its area holds what the case is about, so none passes on an empty mask."""
import numpy as np
import pytest

import area_ref as AR
import gpu_harness as G
import selection_ref as SR
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import frame_rd, scene
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
W, H, SPP, TIME = AR.W, AR.H, 1, 777
DEVICE, MEDIAN = 1, 1
CAM_A = S.default_camera()
CAM_C = R.camera_matrix((3.0, 0.5, 5.0), 0.45, 0.0)
CAM_MESH = R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0)  # with fov 0.5: both meshes, the plane and the sky
OUTLINE, FILL = (200, 255, 160, 0), (96, 40, 90, 250)
ERR_INVALID, ERR_STATE = 1, 3


def rd_of(cam, fov, w=W, h=H):
    return frame_rd(cam, w, h, SPP, TIME, fov)


def handle(T, name="spheres", accel="scan", w=W, h=H):
    sh, tr, ma = scene(name)
    t = T.Tracer(w, h)
    t.set_acceleration(0 if accel == "scan" else 1)
    if accel == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    return t, sh


def check_shapes(t, rect, lasso, ids, n_shapes=7):
    """one coverage call over the planes the handle holds against the restatement -> (counts, summary)"""
    counts, got = t.area_coverage(rect, lasso, options=False)
    want_counts, want = AR.coverage(ids["shape"], rect, lasso, n_shapes)
    assert got == want, (rect, got, want)
    assert np.array_equal(counts, want_counts), (rect, counts, want_counts)
    assert got["hit_pixels"] == counts.sum() and got["area_pixels"] == got["hit_pixels"] + got["miss_pixels"]
    return counts, got


@pytest.fixture(scope="module")
def spheres(T):
    """the sphere scene without its planes (the rays beside the spheres miss) under CAM_A: the handle, its ID planes"""
    sh, tr, ma = scene("spheres")
    keep = np.array([3, 4, 5, 6, 0])  # the floor stays, the two walls go: hits, several shapes and misses in one frame
    t = T.Tracer(W, H)
    t.scene_data = R.scene_data(len(keep))
    t.update_scene(sh[keep], tr, ma)
    counts, s = t.area_coverage((0, 0, W, H), options=rd_of(CAM_A, 0.25))
    assert t.last_area_id_pass()
    ids = t.read_id_pass()
    yield t, ids
    t.close()


# ---- 1. shape coverage, rectangles ------------------------------------------------------------------------------------------------
def test_full_frame_sees_shapes_and_misses(spheres):
    t, ids = spheres
    counts, s = check_shapes(t, (0, 0, W, H), None, ids, 5)
    assert s["distinct"] >= 3 and s["miss_pixels"] >= 50 and s["area_pixels"] == W * H, s
    assert (counts > 0).sum() == s["distinct"] and s["target_pixels"] == 0


@pytest.mark.parametrize("name", sorted(AR.RECTS))
def test_rectangles(name, spheres):
    t, ids = spheres
    rect = AR.RECTS[name]
    counts, s = check_shapes(t, rect, None, ids, 5)
    if name.startswith(("outside", "empty")):
        assert s == dict(area_pixels=0, hit_pixels=0, miss_pixels=0, distinct=0, target_pixels=0) and not counts.any()
    else:
        assert s["area_pixels"] > 0
    if name == "width_65":  # the second wave of a row holds one lane
        assert [xb - xa for (_, xa, xb) in AR.segments(rect, W, H)[:2]] == [64, 1]
    if name in ("frame", "width_65", "odd_x", "beyond"):
        assert s["distinct"] >= 2 and s["hit_pixels"] > 0, (name, s)
    assert not t.last_area_id_pass()  # the planes were kept


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_small_frames(w, h, T):
    t, _ = handle(T, w=w, h=h)
    for rect in [(0, 0, w, h), (0, 0, 1, 1), (-3, -3, 9, 9), (w - 1, h - 1, w, h), (w, 0, w + 2, h)]:
        counts, s = t.area_coverage(rect, options=rd_of(CAM_A, 0.25, w, h))
        ids = t.read_id_pass()
        assert ids["shape"].shape == (h, w)
        want_counts, want = AR.coverage(ids["shape"], rect, None, 7)
        assert s == want and np.array_equal(counts, want_counts), rect
    assert t.area_coverage((0, 0, w, h), options=False)[1]["hit_pixels"] == w * h  # every pixel of these frames is on a shape
    t.close()


# ---- 2. lassos --------------------------------------------------------------------------------------------------------------------
LASSO_CASES = ("concave_L", "concave_U", "bow_tie", "diagonal_through_centres", "zigzag_256", "far_outside", "far_sliver", "convex", "zero_area")


@pytest.fixture(scope="module")
def spheres_c(T):
    t, _ = handle(T)
    t.area_coverage((0, 0, W, H), options=rd_of(CAM_C, 0.35))
    ids = t.read_id_pass()
    yield t, ids
    t.close()


@pytest.mark.parametrize("name", LASSO_CASES)
def test_lassos(name, spheres_c):
    t, ids = spheres_c
    lasso = AR.LASSOS[name]
    for rect in (AR.RECTS["inside"], (0, 0, W, H), AR.RECTS["over_right"]):
        counts, s = check_shapes(t, rect, lasso, ids)
        m = AR.mask(rect, lasso, W, H)
        assert s["area_pixels"] == m.sum()
        if name not in AR.EMPTY and rect != AR.RECTS["over_right"]:
            assert 0 < m.sum() < (rect[2] - rect[0]) * (rect[3] - rect[1]), "the lasso cuts the rectangle"
            assert s["distinct"] >= 2, (name, rect, s)


def test_lasso_mask_on_the_device_equals_the_host_mask(spheres_c):
    """area_pixels is the mask's size: row by row (areas one row high) against the host mask, rows above, across and below the lasso"""
    t, _ = spheres_c
    lasso = AR.LASSOS["bow_tie"]
    m = t.area_mask((0, 0, W, H), lasso, W, H)
    assert np.array_equal(m, AR.mask((0, 0, W, H), lasso, W, H))
    for y in (0, 4, 5, 17, 18, 31, 32, 36):
        assert t.area_coverage((0, y, W, y + 1), lasso, options=False)[1]["area_pixels"] == m[y].sum(), y


# ---- 3. triangle coverage ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_runs(T):
    """per acceleration mode: the ID planes of the mesh scene and the triangle coverage of its larger model under two areas"""
    out = {}
    for accel in ("scan", "sah", "median"):
        t, sh = handle(T, "mesh_smooth", accel)
        t.render_ids(rd_of(CAM_MESH, 0.5))
        ids = t.read_id_pass()
        on = [(ids["shape"] == s).sum() for s in (1, 2)]
        s0 = 1 + int(np.argmax(on))
        n_tri = int(sh["num_triangles"][s0])
        xs = np.nonzero((ids["shape"] == s0).any(axis=0))[0]
        xc = int(xs[len(xs) // 2])
        areas = {"frame": ((0, 0, W, H), None), "strip": ((xc - 1, 0, xc + 2, H), None), "lasso": (AR.RECTS["inside"], AR.LASSOS["bow_tie"])}
        got = {k: t.area_triangle_coverage(s0, n_tri, rect, lasso, options=False) for k, (rect, lasso) in areas.items()}
        out[accel] = (ids, s0, n_tri, areas, got)
        with pytest.raises(T.SrtError) as e:
            t.area_triangle_coverage(0, n_tri, (0, 0, W, H), options=False)  # the plane is no model
        assert e.value.code == ERR_INVALID
        with pytest.raises(T.SrtError) as e:
            t.area_triangle_coverage(s0, n_tri - 1, (0, 0, W, H), options=False)  # one short
        assert e.value.code == ERR_INVALID
        with pytest.raises(T.SrtError) as e:
            t.area_triangle_coverage(3, n_tri, (0, 0, W, H), options=False)  # beyond the scene
        assert e.value.code == ERR_INVALID
        t.close()
    return out


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_triangle_coverage(accel, mesh_runs):
    ids, s0, n_tri, areas, got = mesh_runs[accel]
    assert n_tri == 200
    for k, (rect, lasso) in areas.items():
        want_counts, want = AR.triangle_coverage(ids["shape"], ids["triangle"], s0, n_tri, rect, lasso)
        counts, s = got[k]
        assert s == want and np.array_equal(counts, want_counts), (accel, k)
        assert s["target_pixels"] == counts.sum() > 0 and s["distinct"] == (counts > 0).sum() >= 2
    base = mesh_runs["scan"]
    assert s0 == base[1]
    for k in areas:
        assert np.array_equal(got[k][0], base[4][k][0]) and got[k][1] == base[4][k][1], (accel, k)  # the three give identical counts


def test_triangle_coverage_runs_the_aggregated_rounds_and_the_fallback(mesh_runs):
    """on the device's triangle plane: a 64-pixel row segment of the areas with more distinct triangles of the model than the
    aggregation's round limit (the per-lane atomics run), and one with exactly one key (one round does it all)"""
    ids, s0, n_tri, areas, got = mesh_runs["scan"]
    keys = []
    for rect, _ in (areas["frame"], areas["strip"]):
        for (y, xa, xb) in AR.segments(rect, W, H):
            on = ids["shape"][y, xa:xb] == s0
            keys.append(len(np.unique(ids["triangle"][y, xa:xb][on])))
    assert max(keys) > R.AREA_AGG_ROUNDS, max(keys)
    assert 1 in keys
    assert R.AREA_AGG_ROUNDS == 4


def test_sphere_is_no_model(spheres_c, T):
    t, _ = spheres_c
    with pytest.raises(T.SrtError) as e:
        t.area_triangle_coverage(4, 16, (0, 0, W, H), options=False)
    assert e.value.code == ERR_INVALID


# ---- 4. bounds and state -----------------------------------------------------------------------------------------------------------
def test_capacity_and_state(T):
    t, sh = handle(T)
    lib = t.lib
    a, _ = T.area_record((0, 0, W, H))
    counts, summary = np.full(7, 0xEEEEEEEE, np.uint32), np.zeros((), R.AREA_SUMMARY)
    assert lib.srt_area_coverage(t._h, None, T._ptr(a), None, T._ptr(counts), 7, T._ptr(summary)) == ERR_STATE  # no ID pass yet
    rd = rd_of(CAM_A, 0.25)
    assert lib.srt_area_coverage(t._h, T._ptr(rd), T._ptr(a), None, T._ptr(counts), 6, T._ptr(summary)) == ERR_INVALID  # one short
    assert (counts == 0xEEEEEEEE).all()
    with pytest.raises(T.SrtError):
        t.read_id_pass()  # ... and nothing was launched: there are still no planes
    assert lib.srt_area_coverage(t._h, T._ptr(rd), T._ptr(a), None, T._ptr(counts), 7, None) == ERR_INVALID
    assert lib.srt_area_coverage(t._h, T._ptr(rd), None, None, T._ptr(counts), 7, T._ptr(summary)) == ERR_INVALID
    assert lib.srt_area_coverage(None, T._ptr(rd), T._ptr(a), None, T._ptr(counts), 7, T._ptr(summary)) == ERR_INVALID
    bad, _ = T.area_record((5, 0, 4, 9))
    assert lib.srt_area_coverage(t._h, T._ptr(rd), T._ptr(bad), None, T._ptr(counts), 7, T._ptr(summary)) == ERR_INVALID
    zero = rd.copy()
    zero["width"] = 0
    assert lib.srt_area_coverage(t._h, T._ptr(zero), T._ptr(a), None, T._ptr(counts), 7, T._ptr(summary)) == ERR_INVALID
    with pytest.raises(T.SrtError):
        t.select_area((0, 0, W, H), mode=4)
    got, s = t.area_coverage((0, 0, W, H), options=rd)
    assert t.last_area_id_pass() and s["distinct"] >= 3
    assert np.array_equal(t.area_coverage((0, 0, W, H), options=False)[0], got)
    # a scene with fewer shapes and no new pass: the planes would index another scene
    t.scene_data = R.scene_data(4)
    t.update_scene(sh[:4], *scene("spheres")[1:])
    with pytest.raises(T.SrtError) as e:
        t.area_coverage((0, 0, W, H), options=False, n_shapes=4)
    assert e.value.code == ERR_STATE
    got4, s4 = t.area_coverage((0, 0, W, H), options=rd, n_shapes=4)  # with options the planes are made again
    assert t.last_area_id_pass()
    want4, want_s4 = AR.coverage(t.read_id_pass()["shape"], (0, 0, W, H), None, 4)
    assert np.array_equal(got4, want4) and s4 == want_s4 and not np.array_equal(got4, got[:4])
    t.close()


def test_device_form_stays_inside_its_arrays(T):
    import torch
    t, _ = handle(T)
    t.render_ids(rd_of(CAM_A, 0.25))
    ids = t.read_id_pass()
    guard, n = 0x5EADBEEF, 7
    buf = torch.full((16 + n + 16 + 8 + 16,), guard, dtype=torch.int64, device="cuda").to(torch.int32)  # guards | counts | guards | summary | guards
    torch.cuda.synchronize()
    base = buf.data_ptr()
    for rect, lasso in [((0, 0, W, H), None), (AR.RECTS["inside"], AR.LASSOS["bow_tie"]), (AR.RECTS["outside"], None)]:
        t.area_coverage_device(base + 4 * 16, n, base + 4 * (16 + n + 16), rect, lasso, options=False)
        t.synchronize()
        host = buf.cpu().numpy().view(np.uint32)
        want_counts, want = AR.coverage(ids["shape"], rect, lasso, n)
        assert np.array_equal(host[16:16 + n], want_counts), rect
        s = host[16 + n + 16:16 + n + 16 + 8]
        assert s[:5].tolist() == [want[k] for k in R.AREA_SUMMARY.names[:5]] and not s[5:].any()
        for lo, hi in ((0, 16), (16 + n, 16 + n + 16), (16 + n + 16 + 8, len(host))):
            assert (host[lo:hi] == guard).all(), (rect, lo)
    with pytest.raises(T.SrtError):
        t.area_coverage_device(base + 4 * 16, n - 1, base, (0, 0, W, H), options=False)
    with pytest.raises(T.SrtError):
        t.area_coverage_device(base + 4 * 16 + 2, n, base, (0, 0, W, H), options=False)  # not aligned
    t.close()


# ---- 5. select_area ---------------------------------------------------------------------------------------------------------------
def frame(t, ticks=1):
    t.clear_canvas()
    return t.render(ticks).reshape(t.height, t.width, 4).copy()


def test_select_area_modes_and_the_overlay(T, sky):
    t = G.make(T, sky, scene("spheres"), W, H, spp=SPP, time=TIME)
    t.options = rd_of(CAM_A, 0.25)
    off = frame(t)
    assert len(t.read_selection()) == 0
    rect = (20, 8, 60, 34)
    counts, s = t.area_coverage(rect)
    ids = t.read_id_pass()
    assert np.array_equal(counts, AR.coverage(ids["shape"], rect, None, 7)[0]) and s["distinct"] >= 3
    inside = np.nonzero(counts)[0].tolist()
    t.set_selection([6, 1, 6, 1000], width=3.0, outline=OUTLINE, fill=FILL)
    assert t.read_selection().tolist() == [1, 6, 1000]  # ascending and unique, as given otherwise
    current = [1, 6, 1000]
    for mode in (AR.ADD, AR.SUBTRACT, AR.TOGGLE, AR.REPLACE):
        t.set_selection(current, width=3.0, outline=OUTLINE, fill=FILL)
        n = t.select_area(rect, mode=mode)
        want = AR.combine(current, counts, mode, 1)
        got = t.read_selection()
        assert n == len(want) and np.array_equal(got, want), (mode, got, want)
        assert (np.diff(got.astype(np.int64)) > 0).all()
    assert got.tolist() == inside
    # min_pixels at a shape's exact count (in) and one more (out)
    s4 = int(counts[4])
    assert s4 > 1
    t.select_area(rect, min_pixels=s4)
    assert 4 in t.read_selection()
    t.select_area(rect, min_pixels=s4 + 1)
    assert 4 not in t.read_selection() and len(t.read_selection()) >= 1
    assert t.select_area(rect, min_pixels=0) == len(inside)  # 0 counts as 1
    # the overlaid frame equals the restatement for the list, with the parameters set_selection was given last
    t.select_area((30, 10, 40, 20), AR.LASSOS["convex"])
    sel = t.read_selection()
    assert 4 in sel
    on = frame(t)
    assert t.last_resolve_selected() == (True, False)  # the coverage call's planes serve the overlay
    want, want_alpha, m = SR.apply(off, ids["shape"], sel.tolist(), 7, 3.0, OUTLINE, FILL)
    assert 0.02 <= m.mean() <= 0.9 and np.array_equal(on, want) and np.array_equal(t.read_selection_alpha(), want_alpha)
    assert t.select_area(AR.RECTS["outside"]) == 0 and len(t.read_selection()) == 0  # an empty result: the overlay goes off
    assert np.array_equal(frame(t), off) and t.last_resolve_selected() == (False, False)
    assert t.select_area(rect, mode=AR.ADD) == len(inside)  # ... and ADD starts from nothing
    t.close()


def test_select_area_without_parameters_uses_the_defaults(T, sky):
    t = G.make(T, sky, scene("spheres"), W, H, spp=SPP, time=TIME)
    t.options = rd_of(CAM_A, 0.25)
    off = frame(t)
    assert t.select_area((0, 0, W, H), min_pixels=200) >= 1
    sel = t.read_selection().tolist()
    on = frame(t)
    d = T.selection_defaults()
    want, _, m = SR.apply(off, t.read_id_pass()["shape"], sel, 7, float(d["outline_width"]), tuple(d["outline_argb"]), tuple(d["fill_argb"]))
    assert m.any() and np.array_equal(on, want) and not np.array_equal(on, off)
    t.close()


# ---- 6. left untouched --------------------------------------------------------------------------------------------------------------
def test_coverage_leaves_everything_else_alone(T, sky):
    t = G.make(T, sky, scene("spheres"), W, H, spp=SPP, time=TIME, denoise=dict(iterations=1))
    t.options = rd_of(CAM_A, 0.25)
    t.set_kernel_timers(True)
    t.set_selection([4, 5], width=2.0, outline=OUTLINE, fill=FILL)
    first = frame(t)
    assert t.last_resolve_selected() == (True, True)
    before = (t.counters(), t.read_canvas().copy(), t.read_argb().copy(), t.read_denoised().copy(), t.read_selection().copy(), t.last_trace_launches(),
              t.last_trace_class(), t.last_kernel_ms(), t.last_resolve_selected(), t.last_ray_query_ms())
    counts, s = t.area_coverage((5, 5, 60, 30), AR.LASSOS["bow_tie"])
    assert not t.last_area_id_pass() and s["distinct"] >= 2  # the overlay's planes serve an unchanged camera
    t.area_coverage((0, 0, W, H), options=False)
    assert t.last_area_ms() > 0.0
    after = (t.counters(), t.read_canvas(), t.read_argb(), t.read_denoised(), t.read_selection(), t.last_trace_launches(), t.last_trace_class(),
             t.last_kernel_ms(), t.last_resolve_selected(), t.last_ray_query_ms())
    assert before[0] == after[0] and before[5:] == after[5:]
    for k in (1, 3):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    assert np.array_equal(before[2], after[2]) and np.array_equal(before[4], after[4])
    second = frame(t)
    assert t.last_resolve_selected() == (True, False)  # no ID pass for the repeated frame either
    assert np.array_equal(first, second)
    t.set_kernel_timers(False)
    t.area_coverage((0, 0, W, H))
    assert t.last_area_ms() == 0.0 and not t.last_area_id_pass()
    t.close()


# ---- 7. the group ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_devices", [2, 3])
def test_group_gives_the_single_handles_counts(n_devices, T, sky):
    rd = rd_of(CAM_C, 0.35)
    cases = [((0, 0, W, H), None), (AR.RECTS["inside"], AR.LASSOS["concave_U"]), (AR.RECTS["over_left"], None)]
    single, _ = handle(T)
    want = [single.area_coverage(rect, lasso, options=rd) for rect, lasso in cases]
    single.close()
    g = T.TracerGroup(W, H, n_devices=n_devices, devices=[0] * n_devices, rows_per_block=8)
    g.set_skybox(sky)
    g.options, g.scene_data = rd.copy(), R.scene_data(7)
    g.update_scene(*scene("spheres"))
    g.clear_canvas()
    for (rect, lasso), (counts, s) in zip(cases, want):
        got_counts, got = g.area_coverage(rect, lasso)
        assert got == s and np.array_equal(got_counts, counts), rect
    assert s["distinct"] >= 1 and want[0][1]["distinct"] >= 3
    n = g.select_area((0, 0, W, H), min_pixels=100)
    sel = g.read_selection()
    assert n == len(sel) >= 2 and np.array_equal(sel, AR.combine([], want[0][0], AR.REPLACE, 100))
    g.render(1)
    assert g.last_resolve_selected() == (True, False)  # the group's one ID state: the coverage call's planes serve its overlay
    g.close()


def test_group_triangle_coverage(T, sky, mesh_runs):
    ids, s0, n_tri, areas, got = mesh_runs["scan"]
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
    g.set_skybox(sky)
    sh, tr, ma = scene("mesh_smooth")
    g.options, g.scene_data = rd_of(CAM_MESH, 0.5), R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    rect, lasso = areas["lasso"]
    counts, s = g.area_triangle_coverage(s0, n_tri, rect, lasso)
    assert s == got["lasso"][1] and np.array_equal(counts, got["lasso"][0])
    g.close()


# ---- 8. the headless route ----------------------------------------------------------------------------------------------------------
def test_headless_select_area_prints_the_python_paths_counts(T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    prefix, ppm = str(tmp_path / "s"), tmp_path / "f.ppm"
    lasso = [(10, 2), (66, 6), (60, 35), (14, 30)]
    cmd = [exe, "--scene", "spheres", "--width", str(W), "--height", str(H), "--spp", "1", "--bounces", "2", "--frames", "1", "--select", "1:3",
           "--select-area", "5,3:64,33:add:40", "--lasso", ";".join(f"{x},{y}" for x, y in lasso), "--out", str(ppm), "--dump", prefix]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    t = T.Tracer(W, H)
    t.set_skybox(np.fromfile(prefix + ".sky.bin", np.float32).reshape(1024, 2048, 4))
    t.options = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    shapes = np.fromfile(prefix + ".shapes.bin", R.SHAPE)
    t.scene_data = np.fromfile(prefix + ".sd.bin", R.SCENE_DATA)[0]
    t.update_scene(shapes, np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    counts, s = t.area_coverage((5, 3, 64, 33), lasso)
    want_counts, want = AR.coverage(t.read_id_pass()["shape"], (5, 3, 64, 33), lasso, len(shapes))
    assert np.array_equal(counts, want_counts) and s == want and s["distinct"] >= 2
    printed = {int(a): int(b) for a, b in re.findall(r"^shape (\d+) count (\d+)$", out, re.M)}
    assert printed == {int(i): int(c) for i, c in enumerate(counts) if c}, out
    sel = AR.combine([1], counts, AR.ADD, 40)
    assert f"area selection: {len(sel)} shape(s)\n" in out and f"selection: {len(sel)} shape(s)\n" in out, out
    # the written picture carries the overlay of that list, with --select's width
    t.clear_canvas()
    plain = t.render(1).reshape(H, W, 4).copy()
    t.set_selection(sel.tolist(), width=3.0)
    t.clear_canvas()
    got = t.render(1).reshape(H, W, 4)
    data = ppm.read_bytes()
    header = f"P6 {W} {H} 255\n".encode()
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)
    assert np.array_equal(got[..., 1:], rgb) and not np.array_equal(got, plain)
    t.close()
