"""Nearest-surface queries on the device (include/srt_abi.h "nearest-surface queries"; csrc/nearest.hip): all 8 words of every
record against tests/nearest_ref.py's brute force, under the array scan and every hierarchy; counts and tails, max_distance,
skip_shape, hostile queries, blocks that are not full, refitted and deformed models, materials, what a query leaves untouched,
the group form and the headless route."""
import numpy as np
import pytest

import bvh_deform_cases as D
import bvh_walk_cases as W
import nearest_ref as NR
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import ACCELS, CAMERAS, FH, FW, frame_rd, primary, scene
from simple_raytracer_amd import records as R, scenes as S
from test_gpu_ray_query import handle

pytestmark = pytest.mark.gpu
F = np.float32
SRT_ERR_INVALID = 1
DEVICE, DEFORM_REFIT = 1, 1
NQ = 257
NOTHING = np.zeros((), R.NEAREST)
NOTHING["distance"], NOTHING["shape"], NOTHING["triangle"], NOTHING["material"] = np.inf, R.HIT_NONE, R.HIT_NONE, -1


def words(r):
    return NR.words(r)


def world_vertices(sh, tr):
    """(m, 3, 3) world vertices v0, v0 + e1, v0 + e2 of every model triangle of the scene, as the kernels hold them"""
    out = [np.zeros((0, 3, 3), F)]
    for s in sh:
        if s["type"] == R.SHAPE_MODEL and s["num_triangles"]:
            w = NR.world_records(s, tr)
            out.append(np.stack([w[:, 0:3], w[:, 0:3] + w[:, 3:6], w[:, 0:3] + w[:, 6:9]], 1))
    return np.concatenate(out).astype(F)


def scene_box(sh, tr):
    pts = [world_vertices(sh, tr).reshape(-1, 3)]
    for s in sh:
        if s["type"] == R.SHAPE_SPHERE:
            c, r = s["sphere_position"], abs(float(s["sphere_radius"]))
            pts.append(np.array([c - r, c + r], F))
    pts = np.concatenate(pts)
    pts = pts[np.isfinite(pts).all(1)]
    return pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)


_points = {}


def query_points(key, sh, tr, extra=()):
    """NQ points: random in and around the scene's box, on vertices, edges and faces, 10^3 scene sizes away, and `extra`;
    computed once per scene"""
    if key in _points:
        return _points[key]
    rng = np.random.default_rng(sum(map(ord, key)))
    lo, hi = scene_box(sh, tr)
    size = hi - lo
    wv = world_vertices(sh, tr)
    pts = [np.asarray(extra, F).reshape(-1, 3)]
    if len(wv):
        pick = wv[rng.integers(0, len(wv), 16)]
        pts += [pick[:, 0], pick[:, 1], pick[:, 2], (pick[:, 0] + pick[:, 1]) * F(0.5), (pick[:, 1] + pick[:, 2]) * F(0.5),
                (pick[:, 0] + pick[:, 1] + pick[:, 2]) / F(3)]
    for s in sh[sh["type"] == R.SHAPE_SPHERE][:6]:
        pts.append((s["sphere_position"] + np.array([[abs(float(s["sphere_radius"])), 0, 0], [0, 0, 0]], F)).astype(F))
    centre = (lo + hi) / 2
    far = rng.normal(size=(16, 3))
    pts.append(centre + far / np.linalg.norm(far, axis=1, keepdims=True) * np.linalg.norm(size) * 1e3)
    have = sum(len(p) for p in pts)
    pts.append(rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (NQ - have, 3)))
    out = np.concatenate([np.asarray(p, F) for p in pts]).astype(F)
    assert out.shape == (NQ, 3)
    _points[key] = out
    return out


_refs = {}


def reference(key, sh, tr, pts, **kw):
    k = (key, tuple(sorted((a, str(b) if not np.isscalar(b) and b is not None else b) for a, b in kw.items() if a != "tri_materials")))
    if k not in _refs or "tri_materials" in kw:
        ref = NR.brute_force(sh, tr, R.point_queries(pts), **kw)
        if "tri_materials" in kw:
            return ref
        _refs[k] = ref
    return _refs[k]


def check(got, want, what):
    bad = np.nonzero((words(got) != words(want)).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


# ---- 1. against the brute force, every word ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [(n, a) for n in ("spheres", "boxes", "mesh_smooth", "mesh_flat") for a in ACCELS[n]])
def test_records_equal_the_brute_force(name, accel, T):
    sh, tr, ma = scene(name)
    extra = [s["transform"][3, :3] for s in sh if s["type"] == R.SHAPE_MODEL and s["num_triangles"] == 12][:4]  # box centres: exact ties
    pts = query_points(name, sh, tr, extra)
    want = reference(name, sh, tr, pts)
    found = (want["flags"] & R.NEAREST_FOUND) != 0
    assert found.all() and len(set(want["shape"].tolist())) >= 2
    if name == "boxes":
        assert len(extra) >= 2 and (want["distance"][:len(extra)] == 1).sum() >= 2  # the centre of a 2-cube: twelve triangles, many at exactly 1
    t = handle(T, name, accel)
    got = t.nearest_points(pts)
    assert got.dtype == R.NEAREST and len(got) == NQ
    check(got, want, (name, accel))
    assert t.counters()["watchdog"] == 0
    t.close()


@pytest.mark.parametrize("mesh,accel", [(m, a) for m in W.MESH_NAMES for a in ("scan", "sah", "median")])
def test_walk_meshes_equal_the_brute_force(mesh, accel, T):
    sc = W.scene(mesh)
    sh, tr, ma = sc["shapes"], sc["tris"], sc["mats"]
    pts = query_points("walk_" + mesh, sh[:1], tr)  # around the mesh (the sphere about it is 8 across)
    want = reference("walk_" + mesh, sh, tr, pts)
    feats = set((((want["flags"] & R.NEAREST_FEATURE_MASK) >> R.NEAREST_FEATURE_SHIFT)[want["shape"] == 0]).tolist())
    assert (want["shape"] == 0).sum() >= 100 and len(feats) >= 4, feats
    t = handle(T, (sh, tr, ma), accel)
    check(t.nearest_points(pts), want, (mesh, accel))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 2. counts and tails -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_form_counts_and_tails(n, T):
    import torch
    sh, tr, ma = scene("mesh_smooth")
    pts = query_points("mesh_smooth", sh, tr)[:n]
    want = reference("mesh_smooth", sh, tr, query_points("mesh_smooth", sh, tr))[:n]
    qs = R.point_queries(pts)
    t = handle(T, "mesh_smooth", "sah")
    dev = torch.device("cuda", 0)
    q_dev = torch.from_numpy(qs.view(np.int32).reshape(n, 4).copy()).to(dev)
    pattern = np.int32(0x5A5A5A5A)
    out_dev = torch.full((n + 64, 8), int(pattern), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.nearest_points_device(q_dev.data_ptr(), n, out_dev.data_ptr())
    t.synchronize()
    got = out_dev.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), words(want))
    assert (got[n:] == pattern).all()
    check(t.nearest_points(pts), want, ("host form", n))
    assert t.counters()["watchdog"] == 0
    t.close()


def test_counts_and_argument_errors_on_a_handle(T):
    t = handle(T, "spheres")
    n_shapes = len(scene("spheres")[0])
    assert len(t.nearest_points(np.zeros((0, 3), F))) == 0
    qs, out = R.point_queries([(0, 0, 0)]), np.zeros(1, R.NEAREST)
    p, lib, h = T._ptr, t.lib, t._h
    assert lib.srt_nearest_points(h, None, 0, R.HIT_NONE, None) == 0 and lib.srt_nearest_points_device(h, None, 0, R.HIT_NONE, None) == 0
    assert lib.srt_nearest_points(h, None, 1, R.HIT_NONE, p(out)) == SRT_ERR_INVALID and lib.srt_nearest_points(h, p(qs), 1, R.HIT_NONE, None) == SRT_ERR_INVALID
    assert lib.srt_nearest_points_device(h, None, 1, R.HIT_NONE, None) == SRT_ERR_INVALID
    assert lib.srt_nearest_points_device(h, 8, 1, R.HIT_NONE, 16) == SRT_ERR_INVALID and b"aligned" in lib.srt_last_error(h)
    assert lib.srt_nearest_points(h, p(qs), 1, n_shapes, p(out)) == SRT_ERR_INVALID and b"skip_shape" in lib.srt_last_error(h)
    assert lib.srt_nearest_points(h, p(qs), 1 << 31, R.HIT_NONE, p(out)) == SRT_ERR_INVALID
    assert not out.view(np.uint32).any()
    assert lib.srt_nearest_points(h, p(qs), 1, n_shapes - 1, p(out)) == 0 and out["flags"][0] & R.NEAREST_FOUND
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 3. max_distance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "scan"), ("mesh_smooth", "sah"), ("mesh_smooth", "median")])
def test_max_distance_is_a_strict_limit(name, accel, T):
    sh, tr, ma = scene(name)
    pts = query_points(name, sh, tr)[-64:]  # (the random ones)
    base = reference(name, sh, tr, query_points(name, sh, tr))[-64:]
    d = base["distance"]
    assert (d > 0).sum() >= 32
    t = handle(T, name, accel)
    nothing = np.tile(words(NOTHING), (64, 1))
    for limit, found in ((np.full(64, np.inf, F), True), (np.full(64, 1e-30, F), False), (d, False), (np.nextafter(d, F(np.inf)), True), (np.nextafter(d, F(-np.inf)), False), (np.zeros(64, F), False),
                         (np.full(64, -0.0, F), False), (np.full(64, -np.inf, F), False)):
        got = t.nearest_points(R.point_queries(pts, limit))
        keep = d > 0 if limit is d or not found else np.ones(64, bool)  # (a point ON a surface has distance 0: nothing is below a limit of 0)
        want = words(base) if found else nothing
        assert np.array_equal(words(got)[keep], want[keep]), (name, accel, float(limit[0]), found)
        check(got, NR.brute_force(sh, tr, R.point_queries(pts, limit)), (name, accel, "limit", float(limit[0])))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 4. skip_shape ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "scan"), ("mesh_smooth", "sah")])
def test_skip_shape_gives_the_second_answer(name, accel, T):
    sh, tr, ma = scene(name)
    pts = query_points(name, sh, tr)
    base = reference(name, sh, tr, pts)
    t = handle(T, name, accel)
    models = np.flatnonzero(sh["type"] == R.SHAPE_MODEL)
    skips = [int(np.bincount(base["shape"]).argmax())] + ([int(m) for m in models] if name != "spheres" else [])
    if name != "spheres":
        assert len(models) == 2 and models[1] == models[0] + 1  # one block holds both: either half is left out alone
    for skip in dict.fromkeys(skips):
        want = reference(name, sh, tr, pts, skip_shape=skip)
        assert (base["shape"] == skip).any() and not (want["shape"] == skip).any()
        check(t.nearest_points(pts, skip_shape=skip), want, (name, accel, skip))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 5. hostile queries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_hostile_queries_get_the_nothing_record(accel, T):
    sh, tr, ma = scene("mesh_smooth")
    qs = R.point_queries(np.tile(np.asarray((0.1, 0.4, 0.2), F), (8, 1)))
    qs["point"][0, 1] = np.nan
    qs["point"][1, 2] = np.inf
    qs["point"][2, 0] = -np.inf
    qs["max_distance"][3] = np.nan
    qs["point"][5] = np.nan
    qs["max_distance"][6] = np.inf
    t = handle(T, "mesh_smooth", accel)
    got = t.nearest_points(qs)
    bad = [0, 1, 2, 3, 5]
    want = NOTHING.copy()
    want["flags"] = R.NEAREST_INVALID
    assert np.array_equal(words(got[bad]), np.tile(words(want), (len(bad), 1)))
    check(got, NR.brute_force(sh, tr, qs), accel)
    assert (got["flags"][[4, 6, 7]] & R.NEAREST_FOUND).all()
    assert t.counters()["watchdog"] == 0
    t.close()


def test_every_query_finds_nothing_before_a_scene_is_set(T):
    t = T.Tracer(FW, FH)
    got = t.nearest_points([(0, 0, 5), (0, 0, 0), (1e6, 2, 3)])
    assert np.array_equal(words(got), np.tile(words(NOTHING), (3, 1)))
    t.close()


# ---- 6. a block that is not full: no filler is ever a candidate ---------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_fillers_are_never_reported(accel, T):
    tris = R.as_records(S.blob_mesh(6, 7, seed=3), R.TRIANGLE)
    ma = np.zeros(2, R.MATERIAL)
    ma[0], ma[1] = R.material((0.8, 0.7, 0.6)), R.material((0.2, 0.7, 0.6))
    sh = np.zeros(5, R.SHAPE)
    # everything well away from the origin, where a filler sphere (centre 0) and the zero padding triangles would sit
    sh[0], sh[1], sh[2] = R.sphere(0, (5, 5, 5), 1.0), R.sphere(1, (-6, 5, 4), 0.5), R.sphere(0, (5, -7, 5), 2.0)
    sh[3] = R.plane(1, (0, -20, 0), (0.5, 2, -0.25))  # n as stored, not unit: k / sqrt(nn) and k / nn on the device too
    sh[4] = R.model(0, tris, 0, len(tris), R.translate((-5, -5, -5)))
    pts = np.concatenate([np.zeros((1, 3), F), np.array([(1e6, 0, 0), (0, 1e6, 0), (-1e6, -1e6, 1e6), (0, -1e6, 0)], F),
                          np.array([(-6, 5, 4), (-6.2, 5.9, 4), (5, -7, 5), (5.5, -9.5, 5)], F), query_points("fillers", sh, tris)[:55]]).astype(F)
    want = NR.brute_force(sh, tris, R.point_queries(pts))
    assert ((want["flags"] & R.NEAREST_FOUND) != 0).all() and set(want["shape"].tolist()) == {0, 1, 2, 3, 4} and want["distance"][0] > 3
    t = handle(T, (sh, tris, ma), accel)
    got = t.nearest_points(pts)
    assert (got["shape"] < 5).all()
    check(got, want, accel)
    for skip in range(5):
        check(t.nearest_points(pts[:5], skip_shape=skip), NR.brute_force(sh, tris, R.point_queries(pts[:5]), skip_shape=skip), (accel, "skip", skip))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 7. refitted and deformed models ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sah", "median"])
def test_a_query_sees_the_device_refit(kind, T):
    sh, tr, ma = scene("mesh_smooth")
    t = handle(T, "mesh_smooth", kind, refit=True)
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    pts = query_points("mesh_smooth", sh, tr)
    want = NR.brute_force(moved, tr, R.point_queries(pts))
    assert (words(want) != words(reference("mesh_smooth", sh, tr, pts))).any()
    check(t.nearest_points(pts), want, ("refit", kind))
    assert t.counters()["watchdog"] == 0
    t.close()


def test_a_query_sees_the_deform_refit(T):
    sh, tr, ma = scene("mesh_smooth")
    t = T.Tracer(FW, FH)
    t.set_acceleration(1)
    t.set_acceleration_refit(DEVICE)
    t.set_acceleration_deform(DEFORM_REFIT, 0.0)
    t.options = frame_rd(S.default_camera())
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    first, n = int(sh["triangle_index"][m]), int(sh["num_triangles"][m])
    tr2 = tr.copy()
    tr2[first:first + n] = D.wave(tr[first:first + n])
    sh2 = sh.copy()
    sh2[m] = R.model(int(sh["material"][m]), tr2, first, n, sh["transform"][m])
    t.update_scene(sh2, tr2, ma)
    assert t.acceleration_deform_info()["models_kept"] >= 1
    pts = query_points("mesh_smooth", sh, tr)
    want = NR.brute_force(sh2, tr2, R.point_queries(pts))
    assert (words(want) != words(reference("mesh_smooth", sh, tr, pts))).any()
    check(t.nearest_points(pts), want, "deform refit")
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 8. materials ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_materials_follow_the_casts_rule(accel, T):
    sh, tr, ma = scene("mesh_smooth")
    pts = query_points("mesh_smooth", sh, tr)
    tm = np.full(len(tr), -1, np.int32)
    tm[::3] = 1
    tm[1::3] = 0
    t = handle(T, "mesh_smooth", accel)
    t.set_triangle_materials(tm)
    want = NR.brute_force(sh, tr, R.point_queries(pts), tri_materials=tm)
    plain = reference("mesh_smooth", sh, tr, pts)
    assert (want["material"] != plain["material"]).any() and (want["material"] == plain["material"]).any()
    check(t.nearest_points(pts), want, (accel, "per-triangle"))
    # a shape without a material is still reported, with -1, whatever the table says
    bare = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    bare["material"][m] = -1
    t.update_scene(bare, tr, ma)
    want = NR.brute_force(bare, tr, R.point_queries(pts), tri_materials=tm)
    on = want["shape"] == m
    assert on.sum() >= 8 and (want["material"][on] == -1).all() and ((want["flags"][on] & R.NEAREST_FOUND) != 0).all()
    check(t.nearest_points(pts), want, (accel, "no material"))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 9. state ----------------------------------------------------------------------------------------------------------------------------------
def test_a_query_leaves_the_frame_alone(T, sky):
    sh, tr, ma = scene("mesh_smooth")
    cam = CAMERAS["mesh_smooth"][0]
    t = handle(T, "mesh_smooth", "sah", sky=sky)
    t.options = frame_rd(cam)
    t.set_kernel_timers(True)
    t.clear_canvas()
    t.trace()

    def state():
        return (t.read_canvas().view(np.uint32).copy(), t.counters(), t.debug_counters(), t.last_trace_launches(), t.last_trace_kernel_ms(),
                t.last_kernel_ms(), t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured())

    before = state()
    pts = query_points("mesh_smooth", sh, tr)
    got = t.nearest_points(pts)
    assert t.last_ray_query_ms() > 0.0
    after = state()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    check(got, reference("mesh_smooth", sh, tr, pts), "after a frame")
    assert t.counters()["watchdog"] == 0
    t.close()


@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "sah")])
def test_interleaved_with_casts_equals_fresh_handles(name, accel, T):
    """the staging allocation is shared with the casts (csrc/query_stage.h): counts growing and shrinking, each call against the
    same call on a fresh handle"""
    sh, tr, ma = scene(name)
    pts = query_points(name, sh, tr)
    cam = CAMERAS[name][0]
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(NQ, 3)).astype(F)
    calls = [("nearest 257", lambda t: t.nearest_points(pts)), ("cast 65", lambda t: t.cast_rays(cam[3, :3], dirs[:65])),
             ("nearest 1", lambda t: t.nearest_points(pts[7:8], max_distance=50.0)), ("cast 257", lambda t: t.cast_rays(cam[3, :3], dirs)),
             ("nearest 65", lambda t: t.nearest_points(pts[100:165], skip_shape=0)), ("pick 1", lambda t: t.pick([[3.5, 1.5]], options=frame_rd(cam))),
             ("nearest 64", lambda t: t.nearest_points(pts[:64]))]
    one = handle(T, name, accel)
    for what, call in calls:
        got = call(one)
        fresh = handle(T, name, accel)
        want = call(fresh)
        fresh.close()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, accel, what)
    check(one.nearest_points(pts), reference(name, sh, tr, pts), "at the end")
    assert one.counters()["watchdog"] == 0
    one.close()


# ---- 10. group and headless ----------------------------------------------------------------------------------------------------------------------
def test_group_form_gives_the_single_handles_records(T):
    sh, tr, ma = scene("mesh_smooth")
    pts = query_points("mesh_smooth", sh, tr)
    g = T.TracerGroup(FW, FH, n_devices=2, devices=[0, 0], rows_per_block=1)
    g.set_acceleration(1)
    g.scene_data = R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    check(g.nearest_points(pts), reference("mesh_smooth", sh, tr, pts), "group")
    check(g.nearest_points(pts[:9], max_distance=0.75, skip_shape=1), NR.brute_force(sh, tr, R.point_queries(pts[:9], 0.75), skip_shape=1), "group, limits")
    g.close()


def test_headless_nearest_prints_the_record_python_gets(T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    w, h = 32, 24
    asks = [((0.5, 3.0, -3.0), None, None), ((0.0, 0.0, 0.0), 0.25, None), ((2.0, 1.0, -4.0), 100.0, 4), ((0.5, 0.8, -3.0), None, None)]
    prefix = str(tmp_path / "p")
    cmd = [exe, "--scene", "spheres", "--width", str(w), "--height", str(h), "--spp", "1", "--bounces", "1", "--frames", "1", "--dump", prefix]
    for p, radius, skip in asks:
        cmd += ["--nearest", ",".join(map(str, p)) + (f":{radius}" if radius is not None else "") + (f":{skip}" if skip is not None else "")]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("nearest ")]
    assert len(lines) == len(asks), out
    sh, tr, ma = (np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    t = handle(T, (sh, tr, ma), w=w, h=h)
    seen = set()
    for line, (p, radius, skip) in zip(lines, asks):
        want = t.nearest_points([p], max_distance=np.inf if radius is None else radius, skip_shape=skip)[0]
        check(np.array([want]), NR.brute_force(sh, tr, R.point_queries([p], np.inf if radius is None else radius), skip_shape=skip), line)
        if not want["flags"] & R.NEAREST_FOUND:
            assert line.endswith(": nothing"), line
            seen.add("nothing")
            continue
        m = re.search(r"shape (\d+) triangle (-?\d+) material (-?\d+) distance (\S+) point (\S+) (\S+) (\S+) (\w+) (\w+)$", line)
        assert m, line
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (int(want["shape"]), -1, int(want["material"])), line
        assert F(m.group(4)) == want["distance"] and [F(m.group(k)) for k in (5, 6, 7)] == list(want["point"]), line
        assert m.group(8) == "face" and m.group(9) == ("back" if want["flags"] & R.NEAREST_BACK else "front"), line
        seen.add(m.group(9))
    assert {"front", "back"} <= seen, (seen, out)
    t.close()
