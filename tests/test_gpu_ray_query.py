"""Ray queries on the device (include/srt_abi.h "ray queries"; csrc/ray_query.hip): cast_rays and pick against the CPU oracle's
primary hits bit for bit, the record's indices against the denoiser's id planes, the BVH walk against the array scan on the
directed walk cases, counts and tails, tmax, hostile rays, what a query leaves untouched, and the group forms."""
import numpy as np
import pytest

import bvh_walk_cases as W
import gpu_harness as G
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import ACCELS, CAMERAS, FH, FW, NS, TIME, close_mesh, frame_rd, jitter_xy, o_hits, primary, scene, sphere_closeup
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
SRT_ERR_INVALID = 1
DEVICE, MEDIAN = 1, 1  # SRT_BUILD_DEVICE, SRT_BUILD_ORDER_MEDIAN; also SRT_REFIT_DEVICE
MISS = np.zeros((), R.RAY_HIT)
MISS["t"], MISS["shape"], MISS["triangle"], MISS["material"] = np.inf, R.HIT_NONE, R.HIT_NONE, -1


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


def words(h):
    return np.ascontiguousarray(h).view(np.uint32).reshape(-1, 8)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def check_against_oracle(hits, ph, what):
    hit = np.isfinite(ph["t"])
    assert np.array_equal((hits["flags"] & R.HIT_HIT) != 0, hit), what
    assert np.array_equal(np.isfinite(hits["t"]), hit), what
    assert not (hits["flags"] & R.HIT_INVALID_RAY).any(), what
    assert same_bits(hits["t"], ph["t"]), (what, "t")
    assert same_bits(hits["normal"], ph["normal"]), (what, "normal")
    assert np.array_equal(hits["material"], ph["material"]), (what, "material")
    assert np.array_equal(words(hits[~hit]), np.tile(words(MISS), (int((~hit).sum()), 1))), (what, "miss record")
    n = hits["normal"][hit].astype(np.float64)
    # unit length as far as float32 allows: a sphere's normal is (p - c) / r with p = o + d t rounded at the scene's extent (up to 20
    # units from the origin, radii from 0.6), |n|^2 - 1 up to 2 sqrt(3) * 20 * 2^-23 / 0.6 = 1.4e-5; the other kinds are normalised
    assert np.all(np.abs((n * n).sum(axis=1) - 1.0) < 1e-4), what
    assert np.all((n * ph["dir"][hit].astype(np.float64)).sum(axis=1) <= 0.0), (what, "the normal faces the ray")


# ---- 1. against the oracle, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [(n, a) for n in CAMERAS for a in ACCELS[n]])
def test_cast_equals_oracle_primary_hits(name, accel, T, oracle):
    t = handle(T, name, accel)
    for k, cam in enumerate(CAMERAS[name]):
        _, _, ph = primary(oracle, name, k)
        hits = t.cast_rays(cam[3, :3], ph["dir"], unit=True)
        assert hits.dtype == R.RAY_HIT and len(hits) == FW * FH * NS
        check_against_oracle(hits, ph, (name, accel, k))
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 2. pick equals the sample's ray -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("boxes", "sah"), ("mesh_smooth", "median"), ("mesh_flat", "scan")])
def test_pick_equals_the_samples_primary_ray(name, accel, T, oracle):
    t = handle(T, name, accel)
    for k, cam in enumerate(CAMERAS[name]):
        ids, sm, ph = primary(oracle, name, k)
        rd = frame_rd(cam)
        cast = t.cast_rays(cam[3, :3], ph["dir"], unit=True)
        picked = t.pick(jitter_xy(oracle, rd, ids, sm), options=rd)
        assert np.array_equal(words(picked), words(cast)), (name, k)
        check_against_oracle(picked, ph, (name, accel, k, "pick"))
    t.close()


def test_pick_of_pixel_centres_on_the_sphere_scene(T):
    t = handle(T, "spheres")
    cam = S.default_camera()
    # the middle pixel of a 9x5 frame: its centre is the view axis, which meets the sphere at (0.5, 0.8, -3), shape 4
    mid = t.pick([4.5, 2.5], options=frame_rd(cam, 9, 5))[0]
    sh = scene("spheres")[0]
    assert mid["shape"] == 4 and mid["triangle"] == R.HIT_NONE and mid["material"] == sh["material"][4]
    assert mid["flags"] == R.HIT_HIT | R.HIT_FRONT
    assert abs(float(mid["t"]) - (8.0 - np.sqrt(1.0 - 0.25 - 0.09))) < 1e-5
    # the 8x4 frame's pixel centres: the rays numpy forms the same way (to the last bits of the normalisation) see the same shapes
    rec = dict(cam=cam, w=FW, h=FH, fov=1.0)
    org, dirs = W.primary_rays(rec)
    xy = [(px + 0.5, py + 0.5) for py in range(FH) for px in range(FW)]
    picked, cast = t.pick(xy, options=frame_rd(cam)), t.cast_rays(org, dirs)
    assert np.array_equal(picked["shape"], cast["shape"]) and (picked["flags"] & R.HIT_HIT).sum() >= 8
    assert np.allclose(picked["t"], cast["t"], rtol=1e-5)
    t.close()


# ---- 3. shape and triangle indices, materials ----------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_indices_equal_the_denoisers_id_planes(accel, T, sky, oracle):
    sh, tr, ma = scene("mesh_smooth")
    assert (sh["material"] >= 0).all()
    rd, ids, sm, ph = close_mesh(oracle)
    t = G.make(T, sky, (sh, tr, ma), FW, FH, spp=NS, accel=0 if accel == "scan" else 1, time=TIME, denoise=dict(feature_samples=1), temporal={},
               motion=True)
    t.set_denoise_vertex_motion(True)
    t.options = rd
    t.trace()
    t.synchronize()
    shape_ids, _ = t.read_denoise_shape_ids()
    tri_ids, _ = t.read_denoise_triangle_ids()
    s0 = sm == 0
    picked = t.pick(jitter_xy(oracle, rd, ids[s0], sm[s0]))
    assert np.array_equal(picked["shape"], shape_ids.reshape(-1)) and np.array_equal(picked["triangle"], tri_ids.reshape(-1))
    on_model = np.isin(ph["material"][s0], sh["material"][sh["type"] == R.SHAPE_MODEL])  # (the oracle's: the models have materials of their own)
    assert on_model.sum() >= 8 and (~on_model).sum() >= 8
    assert np.array_equal(picked["triangle"] != R.HIT_NONE, on_model)
    assert np.array_equal(sh["type"][picked["shape"][on_model]], np.full(on_model.sum(), R.SHAPE_MODEL))
    t.close()


@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_material_is_the_per_triangle_one(accel, T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    rd, ids, sm, ph = close_mesh(oracle)
    org = rd["camera_to_world"][3, :3]
    t = handle(T, "mesh_smooth", accel)
    before = t.cast_rays(org, ph["dir"], unit=True)
    check_against_oracle(before, ph, "close")
    on_model = np.isin(ph["material"], sh["material"][sh["type"] == R.SHAPE_MODEL])
    assert on_model.sum() >= 16
    m = int(before["shape"][on_model][0])
    j = int(before["triangle"][on_model][0])
    other = (int(sh["material"][m]) + 1) % len(ma)
    tm = np.full(len(tr), -1, np.int32)
    tm[int(sh["triangle_index"][m]) + j] = other
    t.set_triangle_materials(tm)
    after = t.cast_rays(org, ph["dir"], unit=True)
    there = on_model & (before["shape"] == m) & (before["triangle"] == j)
    assert there.any() and (after["material"][there] == other).all()
    assert np.array_equal(after["material"][~there], before["material"][~there])
    for f in ("t", "shape", "triangle", "normal", "flags"):
        assert np.array_equal(after[f], before[f]), f
    t.close()


def test_a_shape_without_a_material_is_reported(T, oracle):
    sh, tr, ma = scene("spheres")
    rd, _, _, ph = sphere_closeup(oracle)
    org = rd["camera_to_world"][3, :3]
    target = 4  # the sphere in the middle of the view, in front of the back wall; the oracle's material is the shape's index here
    assert np.array_equal(sh["material"], np.arange(len(sh)))
    bare = sh.copy()
    bare["material"][target] = -1
    t, u = handle(T, "spheres"), handle(T, (bare, tr, ma))
    with_mat, without = t.cast_rays(org, ph["dir"], unit=True), u.cast_rays(org, ph["dir"], unit=True)
    check_against_oracle(with_mat, ph, "closeup")
    on = with_mat["shape"] == target
    assert on.sum() >= 4 and np.array_equal(on, ph["material"] == target)
    assert (without["material"][on] == -1).all() and ((without["flags"][on] & R.HIT_HIT) != 0).all()
    for f in ("t", "shape", "triangle", "normal", "flags"):
        assert np.array_equal(without[f], with_mat[f]), f
    assert np.array_equal(without["material"][~on], with_mat["material"][~on])
    t.close(), u.close()


# ---- 4. BVH equals scan on the directed walk cases -----------------------------------------------------------------------------
NON_VACUOUS = ("on_plane_in", "axis_parallel")


@pytest.mark.parametrize("kind", W.TREES)
def test_walk_equals_scan_on_the_directed_cases(kind, T, oracle):
    seen = {fam: [0, 0] for fam in NON_VACUOUS}
    failures = []
    for mesh in W.MESH_NAMES:
        sc = W.scene(mesh)
        arrays = (sc["shapes"], sc["tris"], sc["mats"])
        scan, bvh = handle(T, arrays, "scan", w=W.W, h=W.H), handle(T, arrays, kind, w=W.W, h=W.H)
        for fam in NON_VACUOUS:
            for rec in W.oracle_subset(mesh, kind, fam):
                rd = W.render_data(rec)
                ns = int(rd["num_samples"])
                ids, sm = np.repeat(np.arange(W.W * W.H), ns), np.tile(np.arange(ns), W.W * W.H)
                xy = jitter_xy(oracle, rd, ids, sm)
                a, b = scan.pick(xy, options=rd), bvh.pick(xy, options=rd)
                ph = o_hits(oracle, rd, *arrays, ids, sm)
                if not np.array_equal(words(a), words(b)):
                    failures.append((rec["name"], "walk != scan"))
                if not (same_bits(a["t"], ph["t"]) and same_bits(a["normal"], ph["normal"]) and np.array_equal(a["material"], ph["material"])):
                    failures.append((rec["name"], "oracle"))
                seen[fam][0] += int((a["shape"] == 0).any())  # shape 0 is the model
                seen[fam][1] += 1
        scan.close(), bvh.close()
    print(f"model hit in {seen}")
    assert not failures, failures
    for fam, (hit, n) in seen.items():
        assert n >= 6 and 2 * hit >= n, (fam, hit, n)


# ---- 5. counts and tails -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_form_counts_and_tails(n, T, oracle):
    import torch
    cam = CAMERAS["mesh_smooth"][0]
    _, _, ph = primary(oracle, "mesh_smooth", 0)
    rays = R.rays(cam[3, :3], ph["dir"][np.arange(n) % len(ph["dir"])])
    t = handle(T, "mesh_smooth", "sah")
    want = t.cast_rays(rays, unit=True)
    dev = torch.device("cuda", 0)
    rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
    pattern = np.int32(0x5A5A5A5A)
    hits_dev = torch.full((n + 64, 8), int(pattern), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True)
    t.synchronize()
    got = hits_dev.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), words(want))
    assert (got[n:] == pattern).all()
    assert np.array_equal(words(want[:min(n, 64)]), words(t.cast_rays(cam[3, :3], ph["dir"][:min(n, 64)], unit=True)))
    t.close()


def test_counts_and_argument_errors_on_a_handle(T):
    t = handle(T, "spheres")
    assert len(t.cast_rays(np.zeros((0, 3), F), np.zeros((0, 3), F))) == 0 and len(t.pick(np.zeros((0, 2), F))) == 0
    rays, hits = np.zeros(1, R.RAY), np.zeros(1, R.RAY_HIT)
    rd, xy = R.as_records(t.options, R.RENDER_DATA), np.zeros((1, 2), F)
    p, lib, h = T._ptr, t.lib, t._h
    assert lib.srt_cast_rays(h, None, 0, 0, None) == 0 and lib.srt_cast_rays_device(h, None, 0, 0, None) == 0 and lib.srt_pick(h, None, None, 0, None) == 0
    assert lib.srt_cast_rays(h, None, 1, 0, p(hits)) == SRT_ERR_INVALID and lib.srt_cast_rays(h, p(rays), 1, 0, None) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_device(h, None, 1, 0, None) == SRT_ERR_INVALID
    assert lib.srt_cast_rays(h, p(rays), 1, 2, p(hits)) == SRT_ERR_INVALID and lib.srt_cast_rays(h, p(rays), 1, 0x80000001, p(hits)) == SRT_ERR_INVALID
    assert b"flag" in lib.srt_last_error(h)
    assert lib.srt_pick(h, None, p(xy), 1, p(hits)) == SRT_ERR_INVALID and lib.srt_pick(h, p(rd), None, 1, p(hits)) == SRT_ERR_INVALID
    assert lib.srt_pick(h, p(rd), p(xy), 1, None) == SRT_ERR_INVALID
    assert not hits.view(np.uint32).any()
    t.close()


# ---- 6. tmax and normalisation -------------------------------------------------------------------------------------------------
def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, F).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, F).view(np.int32).astype(np.int64))


def test_tmax_and_normalisation(T, oracle):
    cam = CAMERAS["spheres"][0]
    _, _, ph = primary(oracle, "spheres", 0)
    t = handle(T, "spheres")
    base = t.cast_rays(cam[3, :3], ph["dir"], unit=True)
    k = int(np.flatnonzero(base["flags"] & R.HIT_HIT)[0])
    d, t0 = ph["dir"][k], base["t"][k]
    got = t.cast_rays(cam[3, :3], np.tile(d, (5, 1)), tmax=[t0, np.nextafter(t0, F(np.inf)), np.inf, 0.0, -1.0], unit=True)
    assert np.array_equal(words(got[[0, 3, 4]]), np.tile(words(MISS), (3, 1)))  # strictly closer than tmax
    assert np.array_equal(words(got[1:3]), np.tile(words(base[k:k + 1]), (2, 1)))
    # the same rays, their directions scaled by 3 and normalised by the device: normalize3 of a scaled vector may differ in its last bit
    hit = (base["flags"] & R.HIT_HIT) != 0
    scaled = t.cast_rays(cam[3, :3], ph["dir"] * F(3.0))
    diff = ulps(scaled["t"][hit], base["t"][hit])
    print(f"direction x 3, unit=False: t differs by {int(diff[np.flatnonzero(hit) == k][0])} ulps on ray {k}, at most {int(diff.max())} over {int(hit.sum())} hits")
    assert scaled["shape"][k] == base["shape"][k] and ulps(scaled["t"][k], t0) <= 2
    t.close()


# ---- 7. hostile rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_hostile_rays_get_the_miss_record(accel, T, oracle):
    cam = CAMERAS["mesh_smooth"][0]
    _, _, ph = primary(oracle, "mesh_smooth", 0)
    t = handle(T, "mesh_smooth", accel)
    base = t.cast_rays(cam[3, :3], ph["dir"], unit=True)
    k = int(np.flatnonzero(base["flags"] & R.HIT_HIT)[0])
    o, d = cam[3, :3], ph["dir"][k]
    for unit in (True, False):
        rays = R.rays(o, np.tile(d, (9, 1)))
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
        got = t.cast_rays(rays, unit=unit)
        want = MISS.copy()
        want["flags"] = R.HIT_INVALID_RAY
        assert np.array_equal(words(got[bad]), np.tile(words(want), (len(bad), 1))), unit
        if unit:
            assert np.array_equal(words(got[[4, 7, 8]]), np.tile(words(base[k:k + 1]), (3, 1)))  # the valid rays among them
        else:
            assert got["shape"][4] == base["shape"][k] and (got["flags"][4] & R.HIT_HIT)
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 8. state ------------------------------------------------------------------------------------------------------------------
def test_a_query_leaves_the_frame_alone(T, sky, oracle):
    cam = CAMERAS["mesh_smooth"][0]
    _, _, ph = primary(oracle, "mesh_smooth", 0)
    t = handle(T, "mesh_smooth", "sah", sky=sky)
    t.options = frame_rd(cam)
    t.set_kernel_timers(True)
    t.clear_canvas()
    t.trace()

    def state():
        return (t.read_canvas().view(np.uint32).copy(), t.counters(), t.debug_counters(), t.last_trace_launches(), t.last_trace_kernel_ms(),
                t.last_kernel_ms(), t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured())

    before = state()
    hits = t.cast_rays(cam[3, :3], ph["dir"][:64], unit=True)
    picked = t.pick([[3.5, 1.5]])
    assert t.last_ray_query_ms() > 0.0
    after = state()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    assert (hits["flags"] & R.HIT_HIT).any() and len(picked) == 1
    t.close()


def test_every_ray_misses_before_a_scene_is_set(T):
    t = T.Tracer(FW, FH)
    got = t.cast_rays((0, 0, 5), [(0, 0, -1), (0, -1, 0), (1, 2, 3)])
    assert np.array_equal(words(got), np.tile(words(MISS), (3, 1)))
    assert np.array_equal(words(t.pick([[4.0, 2.0]])), words(MISS))
    t.close()


def test_a_cast_sees_the_updated_scene(T, oracle):
    sh, tr, ma = scene("spheres")
    rd, _, _, ph = sphere_closeup(oracle)
    org = rd["camera_to_world"][3, :3]
    t = handle(T, "spheres")
    check_against_oracle(t.cast_rays(org, ph["dir"], unit=True), ph, "before the move")
    moved = sh.copy()
    moved["sphere_position"][4] += np.asarray((0.4, -0.2, 0.3), F)
    t.update_scene(moved, tr, ma)
    ph2 = sphere_closeup(oracle, shapes=moved)[3]
    assert same_bits(ph2["dir"], ph["dir"]) and not same_bits(ph2["t"], ph["t"]) and (ph2["material"] == 4).sum() >= 4
    check_against_oracle(t.cast_rays(org, ph2["dir"], unit=True), ph2, "after the move")
    t.close()


@pytest.mark.parametrize("kind", ["sah", "median"])
def test_a_cast_sees_the_device_refit(kind, T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    cam = CAMERAS["mesh_smooth"][0]
    t = handle(T, "mesh_smooth", kind, refit=True)
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    ph = primary(oracle, "mesh_smooth", 0)[2]
    ph2 = primary(oracle, "mesh_smooth", 0, shapes=moved)[2]
    assert not same_bits(ph2["t"], ph["t"])
    check_against_oracle(t.cast_rays(cam[3, :3], ph2["dir"], unit=True), ph2, "after the refit")
    t.close()


# ---- 9. group ------------------------------------------------------------------------------------------------------------------
def test_group_forms_give_the_single_handles_records(T, oracle):
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
    assert np.array_equal(words(g.cast_rays(cam[3, :3], ph["dir"], unit=True)), words(t.cast_rays(cam[3, :3], ph["dir"], unit=True)))
    assert np.array_equal(words(g.pick(xy, options=rd)), words(t.pick(xy, options=rd)))
    check_against_oracle(g.pick(xy, options=rd), ph, "group pick")
    g.close(), t.close()


# ---- the headless route --------------------------------------------------------------------------------------------------------
def test_headless_pick_prints_the_shape_python_picks(T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    w, h = 64, 48
    picks = [(32.0, 24.0), (10.5, 40.5), (50.25, 12.75), (32.5, 1.5), (20.0, 30.0)]
    prefix = str(tmp_path / "p")
    cmd = [exe, "--scene", "spheres", "--width", str(w), "--height", str(h), "--spp", "1", "--bounces", "1", "--frames", "1", "--dump", prefix]
    for x, y in picks:
        cmd += ["--pick", f"{x},{y}"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("pick ")]
    assert len(lines) == len(picks), out
    sh, tr, ma = (np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    rd = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    t = handle(T, (sh, tr, ma), w=w, h=h)
    want = t.pick(picks, options=rd)
    assert (want["flags"] & R.HIT_HIT).sum() >= 3
    for line, rec in zip(lines, want):
        if rec["flags"] & R.HIT_HIT:
            m = re.search(r": shape (\d+) triangle (-?\d+) material (-?\d+) t (\S+) ", line)
            assert m, line
            assert int(m.group(1)) == rec["shape"] and int(m.group(2)) == -1 and int(m.group(3)) == rec["material"], line
            assert F(m.group(4)) == rec["t"], line
        else:
            assert line.endswith(": miss"), line
    assert "frame(s)" in out  # ... then it rendered as before
    t.close()
