"""GPU: per-triangle motion for the denoiser's temporal stage (srt_set_denoise_vertex_motion) -- the triangle indices of the
feature pass against the oracle, the world-vertex tables against their restatement, the switch off = the library as it
was, deformed frames against tests/vertex_motion_ref.py, the error codes, and quality against the spatial filter while a
mesh waves."""
import json

import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import temporal_ref as TR
import vertex_motion_ref as V
from conftest import bits_equal
from gpu_harness import T, cam_at, guide_scene, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import scenes as S
from test_gpu_denoise_motion import dilate, history, oracle_ids

pytestmark = pytest.mark.gpu


def make_vm(T, sky, scn, w, h, **kw):
    t = make(T, sky, scn, w, h, temporal=kw.pop("temporal", {}), motion=True, **kw)
    t.set_denoise_vertex_motion(True)
    return t


def history_vm(t):
    hist = history(t)
    hist["tris"] = t.read_denoise_triangle_ids()[1]
    return hist


# ---- triangle indices -------------------------------------------------------------------------------------------------------
def id_scene(name):
    if name == "boxes":
        return guide_scene("boxes")
    return (*scene("meshes"), S.default_camera())  # two instances of the 968-triangle mesh


def check_triangle_ids(oracle, t, shapes, tris, mats, w, h, ids, tri_ids):
    hit = oracle.primary_hits(t.options, t.scene_data, shapes, tris, mats, np.arange(w * h), np.zeros(w * h, np.int32))
    org = np.asarray(t.options["camera_to_world"], np.float32)[3, :3]
    ids, tri_ids = ids.ravel(), tri_ids.ravel()
    is_model = (ids != M.NO_SHAPE) & (shapes["type"][np.where(ids != M.NO_SHAPE, ids, 0)] == M.MODEL)
    assert is_model.any() and np.all(tri_ids[~is_model] == V.NO_TRIANGLE)
    rows = V.world_rows(shapes, tris)
    first, _ = V.first_rows(shapes)
    for q in np.flatnonzero(is_model):
        s, j = int(ids[q]), int(tri_ids[q])
        m, n, i0 = shapes[s]["transform"], int(shapes[s]["num_triangles"]), int(shapes[s]["triangle_index"])
        assert j < n, (q, s, j)

        def distance(k):
            p = [oracle.matrix_by_vector(m, np.append(np.asarray(tris["v"]["pos"][i0 + k, c], np.float32)[:3], np.float32(1.0)))[:3] for c in range(3)]
            return oracle.intersect_triangle(p[0], p[1], p[2], org, hit["dir"][q])

        ok, dist = distance(j)
        assert ok and np.float32(dist).tobytes() == np.float32(hit["t"][q]).tobytes(), (q, s, j, dist, hit["t"][q])
        # no triangle of a lower index at the same distance: the oracle's test on those a float64 test puts near it
        if j:
            P = np.float64(rows[first[s]:first[s] + j])
            e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
            d = np.float64(hit["dir"][q])
            pv = np.cross(d, e2)
            with np.errstate(all="ignore"):
                det = np.sum(e1 * pv, 1)
                tt = np.sum(e2 * np.cross(np.float64(org) - P[:, 0], e1), 1) / det
            near = np.flatnonzero(np.abs(tt - float(hit["t"][q])) <= 1e-4 * float(hit["t"][q]))
            for k in near:
                ok_k, dist_k = distance(int(k))
                assert not (ok_k and np.float32(dist_k).tobytes() == np.float32(hit["t"][q]).tobytes()), (q, s, j, int(k))


def run_triangle_ids(T, sky, oracle, name, w, h, accel):
    shapes, tris, mats, cam = id_scene(name)
    t = make_vm(T, sky, (shapes, tris, mats), w, h, spp=1, accel=accel, denoise=dict(iterations=0), cam=cam)
    if name == "mesh968" and h == 3:
        t.options["fov_scale"] = 0.05  # (61x3 is 20 times as wide as high: a narrow lens keeps the meshes several pixels wide)
    for i, (ns, tm) in enumerate(((3, 4096), (2, 31337))):
        t.options["num_samples"] = ns
        t.options["time"] = tm
        t.render(i + 1)
    ids, tri_ids = t.read_denoise_shape_ids()[0], t.read_denoise_triangle_ids()[0]
    assert np.array_equal(ids, oracle_ids(oracle, t, shapes, tris, mats, w, h))
    check_triangle_ids(oracle, t, shapes, tris, mats, w, h, ids, tri_ids)  # the second dispatch's
    t.close()
    return tri_ids


@pytest.mark.parametrize("name", ["boxes", "mesh968"])
@pytest.mark.parametrize("w,h", [(37, 29), (61, 3)])
def test_triangle_ids_equal_oracle_scan_and_bvh(T, sky, oracle, name, w, h):
    scan, bvh = (run_triangle_ids(T, sky, oracle, name, w, h, accel) for accel in (0, 1))
    assert np.array_equal(scan, bvh)
    assert (scan != V.NO_TRIANGLE).any() and (scan == V.NO_TRIANGLE).any()


# ---- the world-vertex tables ------------------------------------------------------------------------------------------------
def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("accel", [0, 1])
def test_vertex_tables_two_instances_over_one_range(T, sky, accel):
    shapes, tris, mats = scene("meshes")
    t = make_vm(T, sky, (shapes, tris, mats), 37, 29, accel=accel, denoise={})
    t.render(1)
    want = V.world_rows(shapes, tris)
    cur, hist = t.read_denoise_vertex_tables()
    assert len(want) == 2 * 968 and same_rows(cur, want) and not hist.any()
    assert not same_rows(want[:968], want[968:])  # two transforms over one range
    t.clear_canvas()
    t2 = V.wave(tris, 12, 968, 1)
    t.update_scene(shapes, t2, mats)
    assert t.read_denoise_history()["valid"]
    table = t.read_denoise_motion()
    assert table["any_moved"] and table["state"].tolist() == [0, V.DEFORMED, V.DEFORMED] and table["first_row"][1:].tolist() == [0, 968]
    assert same_rows(t.read_denoise_vertex_tables()[1], want)  # the history's rows; the frame's are not written by the update
    t.options["time"] += 1
    t.render(1)
    cur, hist = t.read_denoise_vertex_tables()
    assert same_rows(cur, V.world_rows(shapes, t2)) and same_rows(hist, want)
    t.clear_canvas()
    assert same_rows(t.read_denoise_vertex_tables()[1], V.world_rows(shapes, t2))
    t.close()


def test_vertex_table_is_written_at_the_trace_not_at_the_update(T, sky):
    """an update between a frame's last trace and its clear: the frame's table still holds the scene the frame was traced
    with. (Such a frame was on the canvas when the scene changed, so by object motion's rule it does not become a history;
    the next whole frame does, with its own scene's rows.)"""
    shapes, tris, mats = scene("meshes")
    t = make_vm(T, sky, (shapes, tris, mats), 37, 29, accel=1, denoise={})
    t.render(1)
    t.clear_canvas()
    t.update_scene(shapes, tris, mats)
    t.options["time"] += 1
    t.render(1)
    rows_a = V.world_rows(shapes, tris)
    t2 = V.wave(tris, 12, 968, 1)
    t.update_scene(shapes, t2, mats)  # after the last trace, before the clear
    cur, hist = t.read_denoise_vertex_tables()
    assert same_rows(cur, rows_a) and same_rows(hist, rows_a)
    t.clear_canvas()
    assert not t.read_denoise_history()["valid"]  # object motion's rule for a frame that saw two scenes
    t.update_scene(shapes, t2, mats)
    t.render(1)
    assert same_rows(t.read_denoise_vertex_tables()[0], V.world_rows(shapes, t2))
    t.clear_canvas()
    assert t.read_denoise_history()["valid"] and same_rows(t.read_denoise_vertex_tables()[1], V.world_rows(shapes, t2))
    t.close()


# ---- the switch off = the library as it was ---------------------------------------------------------------------------------
def test_switch_off_a_changed_vertex_drops_the_history(T, sky):
    w, h = 37, 29
    shapes, tris, mats = scene("meshes")
    sp = make(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={})
    om = make(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={}, temporal={}, motion=True)
    for k in range(3):
        now = V.wave(tris, 12, 968, k)
        for t in (sp, om):
            t.clear_canvas()
            t.update_scene(shapes, now, mats)
            t.options["time"] = 400 + k
            t.render(1)
        if k:
            assert not om.read_denoise_history()["valid"], k
        assert bits_equal(sp.read_denoised(), om.read_denoised()), k
    with pytest.raises(T.SrtError):
        om.read_denoise_triangle_ids()  # never enabled on this handle
    sp.close()
    om.close()


@pytest.mark.parametrize("steps", [[], [(4, "translate", (0.031, 0.012, 0.02))]], ids=["still", "sphere-moved"])
def test_switch_on_nothing_deformed_equals_object_motion(T, sky, steps):
    w, h = 37, 29
    scn = S.mixed_test_scene() if not steps else S.sphere_scene()
    shapes, tris, mats = scn
    om = make(T, sky, scn, w, h, accel=1, denoise={}, temporal={}, motion=True)
    vm = make_vm(T, sky, scn, w, h, accel=1, denoise={})
    for k in range(5):
        outs = []
        for t in (om, vm):
            t.clear_canvas()
            t.update_scene(M.move_shapes(shapes, tris, steps, k), tris, mats)
            t.options["time"] = 300 + k
            outs.append(t.render(1).copy())
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(om.read_denoised(), vm.read_denoised()), k
        if k:
            a, b = om.read_denoise_motion(), vm.read_denoise_motion()
            assert a["any_moved"] == b["any_moved"] == bool(steps) and a["state"].tolist() == b["state"].tolist()
            assert not (b["state"] == V.DEFORMED).any()
    for t in (om, vm):
        t.clear_canvas()
    a, b = om.read_denoise_history(), vm.read_denoise_history()
    assert a["valid"] and b["valid"] and a["count"].max() > 2
    for key in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(a[key], b[key]), key
    om.close()
    vm.close()


# ---- deformed frames against numpy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.CASES, ids=[c[0] for c in V.CASES])
def test_deformed_frames_match_numpy(T, sky, case):
    """tests/test_vertex_motion_reference.py asserts on the CPU that these deformations flag at most 1 % of a frame's pixels"""
    name, scn_name, accel, upkeep, cam_kind, deform, steps = case
    w, h = V.SIZE
    shapes, tris, mats = V.case_scene(scn_name)
    tp = dict(history_limit=64, normal_threshold=0.9, depth_threshold=0.05)
    t = make_vm(T, sky, (shapes, tris, mats), w, h, accel=accel, denoise=dict(iterations=0), temporal=tp, cam=V.case_camera(scn_name, 0, cam_kind))
    if upkeep:  # the deforming mesh keeps its hierarchy and is refitted on the device
        t.set_acceleration_refit(T.REFIT_DEVICE)
        t.set_acceleration_deform(T.DEFORM_REFIT)
        t.update_scene(shapes, tris, mats)
    t.render(1)
    for k in range(1, V.FRAMES):
        t.clear_canvas()
        hist = history_vm(t)
        assert hist["valid"]
        h_rows = t.read_denoise_vertex_tables()[1]
        now, now_tris = V.case_frame(case, shapes, tris, k)
        prev, prev_tris = V.case_frame(case, shapes, tris, k - 1)
        t.update_scene(now, now_tris, mats)
        assert t.read_denoise_history()["valid"], k  # the deformation kept the history
        table = t.read_denoise_motion()
        want_table = V.scene_table((prev, prev_tris, mats, t.scene_data), (now, now_tris, mats, t.scene_data))
        deformed = want_table["state"] == V.DEFORMED
        assert table["any_moved"] and deformed.any() and table["state"].tolist() == want_table["state"].tolist()
        assert table["first_row"][deformed].tolist() == want_table["first_row"][deformed].tolist()
        table["first_row"] = want_table["first_row"]  # (every shape's, for the restatement's triangle counts)
        assert same_rows(h_rows, V.world_rows(prev, prev_tris))
        t.options["camera_to_world"] = V.case_camera(scn_name, k, cam_kind)
        t.options["time"] = 2000 + k
        argb = t.render(1).copy().reshape(h, w, 4)
        inp = t.read_denoise_inputs()
        ids, tri_ids = t.read_denoise_shape_ids()[0], t.read_denoise_triangle_ids()[0]
        rows = t.read_denoise_vertex_tables()[0]
        assert same_rows(rows, V.world_rows(now, now_tris))
        want = V.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows, **tp)
        got = t.read_denoised()
        t.clear_canvas()
        got_h = t.read_denoise_history()
        t.update_scene(now, now_tris, mats)
        border = want["rep"]["borderline"]
        with np.errstate(all="ignore"):
            ok = np.isclose(got[..., :3], want["c"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= np.isclose(got[..., 3], want["V"], rtol=1e-4, atol=1e-7, equal_nan=True)
            ok &= np.isclose(got_h["count"], want["commit"]["count"], rtol=1e-4)
            ok &= np.isclose(got_h["m1"], want["commit"]["m1"], rtol=1e-4, atol=1e-6, equal_nan=True)
            ok &= np.isclose(got_h["m2"], want["commit"]["m2"], rtol=1e-4, atol=1e-6, equal_nan=True)
            ok &= np.isclose(got_h["colour"], want["commit"]["colour"], rtol=1e-4, atol=1e-6, equal_nan=True).all(-1)
            ok &= (np.abs(argb.astype(int) - D.tonemap(want["c"]).astype(int)) <= 1).all(-1)
        bad = ~ok & ~border
        on = want["rep"]["state"] == V.DEFORMED
        kept = on & (want["h"] > 0) & ~border
        print(f"{name} frame {k}: {int((~ok).sum())} pixels differ ({int(bad.sum())} unflagged), {border.mean() * 100:.3f}% flagged, "
              f"{int(on.sum())} deformed pixels, {int(kept.sum())} with history")
        assert not bad.any(), (k, np.argwhere(bad)[:5])
        assert int((~ok & border).sum()) < 1e-3 * w * h + 1, k
        assert border.mean() <= 0.01, k
        assert kept.any(), k
        assert np.all(got_h["count"][kept] > want["cur"]["P"]), k
    t.close()


def test_waving_mesh_accumulates_history(T, sky):
    """8 frames of a waving mesh at 2 spp: the history count on the mesh's pixels grows past one frame's count"""
    w, h = 37, 29
    shapes, tris, mats = scene("meshes")
    t = make_vm(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={})
    for k in range(8):
        t.clear_canvas()
        t.update_scene(shapes, V.wave(tris, 12, 968, k), mats)
        t.options["time"] = 50 + k
        t.render(1)
        if k:
            assert t.read_denoise_history()["valid"], k
    ids = t.read_denoise_shape_ids()[0]
    t.clear_canvas()
    count = t.read_denoise_history()["count"]
    on = np.isin(ids, [1, 2])
    assert on.sum() > 20 and np.median(count[on]) > 2 and count[on].max() > 8  # one frame's count is 2; eight frames reach 16
    t.close()


def test_error_codes(T, sky):
    scn = S.sphere_scene()
    t = make(T, sky, scn, 32, 24)
    for call in (lambda: t.set_denoise_vertex_motion(True), lambda: t.read_denoise_triangle_ids(), lambda: t.read_denoise_vertex_tables()):
        with pytest.raises(T.SrtError):
            call()
    t.set_denoise()
    t.set_denoise_temporal()
    with pytest.raises(T.SrtError):
        t.set_denoise_vertex_motion(True)  # object motion is off
    with pytest.raises(T.SrtError):
        t.read_denoise_triangle_ids()  # never enabled
    t.set_denoise_object_motion(True)
    t.set_denoise_vertex_motion(True)
    assert t.read_denoise_vertex_tables()[0].shape == (0, 3, 3)  # a scene without models
    t.set_denoise_object_motion(False)  # turns per-triangle motion off with it
    t.set_denoise_object_motion(True)
    t.render(1)
    t.clear_canvas()
    assert t.read_denoise_history()["valid"]
    t.set_denoise_vertex_motion(True)  # a change of the switch drops the history
    assert not t.read_denoise_history()["valid"]
    t.render(1)
    t.clear_canvas()
    assert t.read_denoise_history()["valid"]
    t.set_denoise_vertex_motion(False)
    assert not t.read_denoise_history()["valid"]
    assert t.lib.srt_set_denoise_vertex_motion(None, 1) == 1
    t.close()
    p = make(T, sky, scn, 32, 24)
    p.set_partition(0, 2)
    assert p.lib.srt_set_denoise_vertex_motion(p._h, 1) == 3  # SRT_ERR_STATE on a partitioned handle
    p.close()


# ---- quality while a mesh waves ---------------------------------------------------------------------------------------------
def test_quality_waving_mesh(T, sky):
    """160x90, 8 frames at 2 spp, default filter, camera still, tonemapped MSE against 4096 spp of the last pose; against the
    spatial filter alone, which is what the library delivers for these frames without the switch (asserted). The measured
    ratios: DESIGN.md section 17."""
    w, h, frames = 160, 90, 8
    shapes, tris, mats = scene("meshes")
    at = lambda k: V.wave(tris, 12, 968, k, amplitude=0.04)
    g = make(T, sky, (shapes, at(frames - 1), mats), w, h, spp=4096, accel=1, time=4242)
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    sp = make(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={})
    off = make(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={}, temporal={}, motion=True)
    vm = make_vm(T, sky, (shapes, tris, mats), w, h, accel=1, denoise={})
    for k in range(frames):
        for t in (sp, off, vm):
            t.clear_canvas()
            t.update_scene(shapes, at(k), mats)
            t.options["time"] = 900 + k
            t.render(1)
        if k:
            assert not off.read_denoise_history()["valid"] and vm.read_denoise_history()["valid"], k
    ids = vm.read_denoise_shape_ids()[0]
    a, b, c = (t.read_denoised()[..., :3] for t in (sp, off, vm))
    assert bits_equal(a, c) is False and bits_equal(a, b)  # without the switch a deforming mesh means the spatial filter every frame
    on = np.isin(ids, [1, 2])
    near = dilate(on, 8) & ~on
    mse = lambda x, m: float(np.mean((tone(x)[m] - ref[m]) ** 2))
    everything = np.ones((h, w), bool)
    ratios = {k: mse(c, m) / mse(a, m) for k, m in (("image", everything), ("deformed_shape", on), ("around", near))}
    print("vertex motion quality: " + json.dumps({**ratios, "deformed_pixels": int(on.sum()), "around_pixels": int(near.sum()),
                                                  "mse_spatial": mse(a, everything), "mse_vertex_motion": mse(c, everything)}))
    for t in (sp, off, vm):
        t.close()
    assert on.sum() > 50 and near.sum() > 50
    assert ratios["image"] < 1.0  # the criterion: better than what the library gave before
