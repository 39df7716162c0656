"""Occlusion queries on the device (include/srt_abi.h "occlusion queries"; csrc/occlusion.hip, csrc/device_anyhit.h): the mask
against the CPU oracle's primary hits and against the cast's SRT_HIT_HIT -- the pinned reference -- at the strict bound, on the
directed walk cases, where the early exit takes effect, in the mask's layout, for hostile rays, for segments, for what a query
leaves untouched, and through the group and headless routes."""
import numpy as np
import pytest

import bvh_walk_cases as W
import gpu_harness as G
import occlusion_cases as O
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import ACCELS, CAMERAS, FH, FW, NS, frame_rd, primary, scene
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
SRT_ERR_INVALID = 1
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


def cast_hit(t, rays, unit=True):
    """the pinned reference: SRT_HIT_HIT of srt_cast_rays for the same rays and flags"""
    return (t.cast_rays(rays, unit=unit)["flags"] & R.HIT_HIT) != 0


# ---- 1. against the oracle, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [(n, a) for n in CAMERAS for a in ACCELS[n]])
def test_occluded_equals_oracle_primary_hits(name, accel, T, oracle):
    t = handle(T, name, accel)
    seen = np.zeros(2, int)  # occluded, visible: the two cameras together show both (tests/test_ray_query_host.py)
    for k, cam in enumerate(CAMERAS[name]):
        _, _, ph = primary(oracle, name, k)
        occ, inv = t.occluded_rays(cam[3, :3], ph["dir"], unit=True, with_invalid=True)
        assert occ.dtype == bool and len(occ) == FW * FH * NS
        want = np.isfinite(ph["t"])
        assert np.array_equal(occ, want), (name, accel, k)
        assert not inv.any()
        seen += (want.sum(), (~want).sum())
    assert (seen >= 8).all(), seen
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 2. the strict bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [(n, a) for n in CAMERAS for a in ACCELS[n]])
def test_tmax_is_the_strict_bound(name, accel, T, oracle):
    t = handle(T, name, accel)
    for k, cam in enumerate(CAMERAS[name]):
        _, _, ph = primary(oracle, name, k)
        hit = np.isfinite(ph["t"])
        d, th = ph["dir"][hit], ph["t"][hit].astype(F)
        n = len(th)
        tmaxes = [th, np.nextafter(th, F(np.inf)), F(0.5) * th, np.full(n, -0.0, F), np.zeros(n, F), np.full(n, -np.inf, F)]
        rays = R.rays(cam[3, :3], np.tile(d, (6, 1)), np.concatenate(tmaxes))
        occ, inv = t.occluded_rays(rays, unit=True, with_invalid=True)
        assert np.array_equal(occ, cast_hit(t, rays)), (name, accel, k)
        occ = occ.reshape(6, n)
        assert not occ[0].any(), "a surface at exactly tmax does not occlude"
        assert occ[1].all(), "one ulp further it does"
        assert not occ[2:].any() and not inv.any()  # nothing is closer than the closest hit; tmax <= 0 is not traversed
    t.close()


# ---- 3. walk equals scan on the directed walk cases -------------------------------------------------------------------------------
NON_VACUOUS = ("on_plane_in", "axis_parallel")


@pytest.mark.parametrize("kind", W.TREES)
def test_walk_equals_scan_on_the_directed_cases(kind, T):
    seen = {fam: [0, 0] for fam in NON_VACUOUS}
    failures = []
    for mesh in W.MESH_NAMES:
        sc = W.scene(mesh)
        arrays = (sc["shapes"], sc["tris"], sc["mats"])
        scan, bvh = handle(T, arrays, "scan", w=W.W, h=W.H), handle(T, arrays, kind, w=W.W, h=W.H)
        for fam in NON_VACUOUS:
            for rec in W.oracle_subset(mesh, kind, fam):
                org, dirs = W.primary_rays(rec)
                base = scan.cast_rays(R.rays(org, dirs), unit=True)
                # The scene's second shape is a sphere around the mesh, which every ray meets: with tmax = inf it alone
                # answers. So each ray is also asked with a limit just past its closest hit when that is on the model (shape
                # 0: only the model can occlude) and exactly at it when it is on the sphere (nothing may occlude).
                on_model = ((base["flags"] & R.HIT_HIT) != 0) & (base["shape"] == 0)
                tight = np.where(on_model, np.nextafter(base["t"], F(np.inf)), base["t"]).astype(F)
                for label, tmax in (("inf", np.inf), ("tight", tight)):
                    rays = R.rays(org, dirs, tmax)
                    a, b, c = scan.occluded_rays(rays, unit=True), bvh.occluded_rays(rays, unit=True), cast_hit(scan, rays)
                    if not (np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(c, cast_hit(bvh, rays))):
                        failures.append((rec["name"], label))
                if not np.array_equal(bvh.occluded_rays(R.rays(org, dirs, tight), unit=True), on_model):
                    failures.append((rec["name"], "the model alone"))
                seen[fam][0] += int(on_model.any())
                seen[fam][1] += 1
        scan.close(), bvh.close()
    print(f"model hit in {seen}")
    assert not failures, failures
    for fam, (hit, n) in seen.items():
        assert n >= 6 and 2 * hit >= n, (fam, hit, n)


# ---- 4. the early exit changes nothing ---------------------------------------------------------------------------------------------
def test_early_exit_on_the_sphere_scene(T):
    t = handle(T, "spheres")
    everybody = O.rays_all_behind_the_first_run()
    occ = t.occluded_rays(everybody, unit=True)
    assert occ.all() and np.array_equal(occ, cast_hit(t, everybody))
    one_left = O.rays_one_lane_left(37)
    occ = t.occluded_rays(one_left, unit=True)
    assert np.array_equal(occ, cast_hit(t, one_left)) and not occ[37] and occ.sum() == 63
    later = O.rays_one_lane_for_a_later_run(11)
    occ, hits = t.occluded_rays(later, unit=True), t.cast_rays(later, unit=True)
    assert np.array_equal(occ, (hits["flags"] & R.HIT_HIT) != 0) and occ.all()
    assert hits["shape"][11] == 4 and (hits["shape"][np.arange(64) != 11] != 4).all()
    t.close()


@pytest.mark.parametrize("accel", ["scan", "sah", "median"])
def test_early_exit_with_two_models_in_a_block(accel, T):
    t = handle(T, "mesh_smooth", accel)
    rays = O.rays_two_models()
    hits = t.cast_rays(rays, unit=True)
    assert np.array_equal(hits["shape"], np.tile([1, 2], 32).astype(np.uint32))  # the first model holds the even lanes, the second the odd
    occ = t.occluded_rays(rays, unit=True)
    assert occ.all() and np.array_equal(occ, (hits["flags"] & R.HIT_HIT) != 0)
    # ... and with the odd lanes stopping short of the second model: the first one's answer is the wave's
    short = rays.copy()
    short["tmax"][1::2] = F(0.5) * hits["t"][1::2]
    occ = t.occluded_rays(short, unit=True)
    assert np.array_equal(occ, cast_hit(t, short)) and occ[0::2].all() and not occ[1::2].any()
    t.close()


# ---- 5. the mask's layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_device_form_mask_layout(n, T, oracle):
    import torch
    both = np.concatenate([R.rays(cam[3, :3], primary(oracle, "mesh_smooth", k)[2]["dir"]) for k, cam in enumerate(CAMERAS["mesh_smooth"])])
    rays = both[(np.arange(n) * 37) % len(both)].copy()  # the two cameras' rays mixed: hits and misses in every word
    rays["tmax"][n // 2] = np.nan  # one invalid ray
    t = handle(T, "mesh_smooth", "sah")
    want = cast_hit(t, rays)
    want_inv = np.zeros(n, bool)
    want_inv[n // 2] = True
    assert n == 1 or (want.sum() >= 8 and (~want).sum() >= 8)
    nw, guard = (n + 63) // 64, 4
    dev = torch.device("cuda", 0)
    rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
    pattern = np.int64(0x5A5A5A5A5A5A5A5A)
    for with_invalid in (False, True):
        # one buffer: guard words, the occluded mask, guard words, the invalid mask, guard words
        buf = torch.full((3 * guard + 2 * nw,), int(pattern), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        occ_ptr, inv_ptr = buf.data_ptr() + 8 * guard, buf.data_ptr() + 8 * (2 * guard + nw)
        t.occluded_rays_device(rays_dev.data_ptr(), n, occ_ptr, inv_ptr if with_invalid else None, unit=True)
        t.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        occ_words, inv_words = got[guard:guard + nw], got[2 * guard + nw:2 * guard + 2 * nw]
        assert np.array_equal(occ_words, O.words_of(want)), with_invalid  # tail bits of the last word included: 0
        assert np.array_equal(R.mask_bits(occ_words, n), want)
        rest = np.ones(len(got), bool)
        rest[guard:guard + nw] = False
        if with_invalid:
            assert np.array_equal(inv_words, O.words_of(want_inv))
            rest[2 * guard + nw:2 * guard + 2 * nw] = False
        assert (got[rest] == np.uint64(pattern)).all(), with_invalid  # nothing else was written
    # the host form gives the same bits
    occ, inv = t.occluded_rays(rays, unit=True, with_invalid=True)
    assert np.array_equal(occ, want) and np.array_equal(inv, want_inv)
    t.close()


def test_counts_and_argument_errors_on_a_handle(T):
    import torch
    t = handle(T, "spheres")
    assert len(t.occluded_rays(np.zeros((0, 3), F), np.zeros((0, 3), F))) == 0
    assert len(t.occluded_segments(np.zeros((0, 3), F), np.zeros((0, 3), F))) == 0 and len(t.segment_rays(np.zeros(0, R.SEGMENT))) == 0
    rays, segs, words = np.zeros(1, R.RAY), np.zeros(1, R.SEGMENT), np.zeros(2, np.uint64)
    p, lib, h = T._ptr, t.lib, t._h
    assert lib.srt_occluded_rays(h, None, 0, 0, None, None) == 0 and lib.srt_occluded_rays_device(h, None, 0, 0, None, None) == 0
    assert lib.srt_occluded_segments(h, None, 0, None, None) == 0 and lib.srt_segment_rays(h, None, 0, None) == 0
    assert lib.srt_occluded_rays(h, None, 1, 0, p(words), None) == SRT_ERR_INVALID and lib.srt_occluded_rays(h, p(rays), 1, 0, None, p(words)) == SRT_ERR_INVALID
    assert lib.srt_occluded_rays(h, p(rays), 1, 2, p(words), None) == SRT_ERR_INVALID and b"flag" in lib.srt_last_error(h)
    assert lib.srt_occluded_rays(h, p(rays), 1 << 31, 0, p(words), None) == SRT_ERR_INVALID
    assert lib.srt_occluded_segments(h, None, 1, p(words), None) == SRT_ERR_INVALID and lib.srt_occluded_segments(h, p(segs), 1, None, None) == SRT_ERR_INVALID
    assert lib.srt_segment_rays(h, p(segs), 1, None) == SRT_ERR_INVALID and lib.srt_segment_rays(h, None, 1, p(rays)) == SRT_ERR_INVALID
    dev = torch.zeros(64, dtype=torch.int64, device=torch.device("cuda", 0))
    base = dev.data_ptr()
    assert lib.srt_occluded_rays_device(h, None, 1, 0, base + 256, None) == SRT_ERR_INVALID
    assert lib.srt_occluded_rays_device(h, base, 1, 0, None, None) == SRT_ERR_INVALID
    assert lib.srt_occluded_rays_device(h, base + 8, 1, 0, base + 256, None) == SRT_ERR_INVALID  # rays: 16 bytes
    assert lib.srt_occluded_rays_device(h, base, 1, 0, base + 260, None) == SRT_ERR_INVALID      # masks: 8 bytes
    assert lib.srt_occluded_rays_device(h, base, 1, 0, base + 256, base + 268) == SRT_ERR_INVALID
    assert b"align" in lib.srt_last_error(h)
    assert lib.srt_occluded_rays_device(h, base, 1, 0, base + 264, base + 272) == 0  # 8-byte aligned masks are enough
    t.synchronize()
    assert not words.any()
    t.close()


# ---- 6. hostile rays -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["scan", "sah"])
def test_hostile_rays_are_invalid_and_not_occluded(accel, T, oracle):
    cam = CAMERAS["mesh_smooth"][0]
    _, _, ph = primary(oracle, "mesh_smooth", 0)
    t = handle(T, "mesh_smooth", accel)
    k = int(np.flatnonzero(np.isfinite(ph["t"]))[0])
    for unit in (True, False):
        hostile, bad = O.hostile_rays(cam[3, :3], ph["dir"][k], unit)
        # in one wave with the frame's rays, which must get the answers they get alone
        rays = np.concatenate([R.rays(cam[3, :3], ph["dir"][:26]), hostile, R.rays(cam[3, :3], ph["dir"][26:52])])
        is_bad = np.zeros(len(rays), bool)
        is_bad[26 + np.asarray(bad)] = True
        occ, inv = t.occluded_rays(rays, unit=unit, with_invalid=True)
        assert np.array_equal(inv, is_bad), unit
        assert not occ[is_bad].any(), unit
        assert np.array_equal(occ, cast_hit(t, rays, unit=unit)), unit
        alone = np.concatenate([t.occluded_rays(rays[:26], unit=unit), t.occluded_rays(rays[38:], unit=unit)])
        assert np.array_equal(occ[:26], alone[:26]) and np.array_equal(occ[38:], alone[26:])
        assert occ[26 + 4] and occ[26 + 11]  # the sound rays among the hostile ones hit what ray k hits
    assert t.counters()["watchdog"] == 0
    t.close()


# ---- 7. segments -----------------------------------------------------------------------------------------------------------------
def test_segments_equal_their_rays_word_for_word(T):
    t = handle(T, "mesh_smooth", "sah")
    segs = O.random_segments()
    rays = t.segment_rays(segs)
    a, ai = t.occluded_segments(segs, with_invalid=True)
    b, bi = t.occluded_rays(rays, unit=True, with_invalid=True)
    assert np.array_equal(O.words_of(a), O.words_of(b)) and np.array_equal(O.words_of(ai), O.words_of(bi))
    assert a.any() and (~a).any() and not ai.any()
    assert np.array_equal(a, cast_hit(t, rays))
    t.close()


def test_segment_rays_against_float64(T):
    t = handle(T, "spheres")
    segs = O.random_segments()
    rays = t.segment_rays(segs)
    direction, tmax, dir_bound, tmax_bound = O.segment_rays_f64(segs)
    dir_err, tmax_err = np.abs(rays["direction"] - direction), np.abs(rays["tmax"] - tmax)
    print(f"direction: worst error / bound {np.max(dir_err / dir_bound):.3f}; tmax: {np.max(tmax_err / tmax_bound):.3f}")
    assert np.array_equal(rays["origin"], segs["from"]) and not rays["reserved"].any()
    assert (dir_err <= dir_bound).all() and (tmax_err <= tmax_bound).all()
    t.close()


def test_segments_on_the_sphere_scene(T):
    t = handle(T, "spheres")
    segs, answers = O.sphere_segments()
    occ, inv = t.occluded_segments(segs, with_invalid=True)
    got = ["invalid" if i else "occluded" if o else "visible" for o, i in zip(occ, inv)]
    assert got == answers
    rays = t.segment_rays(segs)
    assert ((t.cast_rays(rays, unit=True)["flags"] & R.HIT_INVALID_RAY) != 0).tolist() == [a == "invalid" for a in answers]
    # a reserved field that is not 0 is refused as well
    spoilt = segs[:1].copy()
    spoilt["reserved"] = 1.0
    assert t.occluded_segments(spoilt, with_invalid=True)[1].all()
    # the keyword form
    assert t.occluded_segments(O.A, (0.5, 0.8, -2.05), 0.0)[0] and not t.occluded_segments(O.A, (0.5, 0.8, -2.05), 0.1)[0]
    t.close()


# ---- 8. state --------------------------------------------------------------------------------------------------------------------
def test_a_query_leaves_the_frame_alone(T, sky, oracle):
    cam = CAMERAS["mesh_smooth"][0]
    _, _, ph = primary(oracle, "mesh_smooth", 0)
    t = G.make(T, sky, scene("mesh_smooth"), FW, FH, spp=NS, accel=1, cam=cam, denoise=dict(feature_samples=1))
    t.set_kernel_timers(True)
    t.trace()

    def state():
        dn = t.read_denoise_inputs()
        return ([t.read_canvas().view(np.uint32).copy()] + [dn[k].view(np.uint32).copy() for k in ("normal_depth", "albedo_hits", "moments")],
                (dn["T"], dn["P"], t.counters(), t.debug_counters(), t.last_trace_launches(), t.last_trace_kernel_ms(), t.last_kernel_ms(),
                 t.last_trace_class(), t.last_trace_plane_form(), t.last_trace_textured()))

    before = state()
    occ = t.occluded_rays(cam[3, :3], ph["dir"][:64], unit=True)
    assert t.last_ray_query_ms() > 0.0
    seg = t.occluded_segments(O.random_segments(65))
    assert t.last_ray_query_ms() > 0.0
    t.segment_rays(O.random_segments(3))
    after = state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1]
    assert occ.any() and len(seg) == 65
    t.trace()  # and the next dispatch runs as if nothing had been asked
    t.synchronize()
    t.close()


def test_every_ray_is_visible_before_a_scene_is_set(T):
    t = T.Tracer(FW, FH)
    occ, inv = t.occluded_rays((0, 0, 5), [(0, 0, -1), (0, -1, 0), (1, 2, 3), (0, 0, 0)], with_invalid=True)
    assert not occ.any() and inv.tolist() == [False, False, False, True]
    assert not t.occluded_segments((0, 0, 5), [(0, 0, -5), (3, 3, 3)]).any()
    t.close()


def test_a_query_sees_the_updated_scene(T):
    sh, tr, ma = scene("spheres")
    t = handle(T, "spheres")
    # towards the middle sphere, ending at the depth of its centre: three units in front of the back wall
    dirs = O.fan((0.5, 0.8, -3.0), 0.3)
    rays = R.rays(O.EYE, dirs, np.float32(np.linalg.norm(np.asarray((0.5, 0.8, -3.0)) - O.EYE)))
    assert (t.cast_rays(rays, unit=True)["shape"] == 4).all() and t.occluded_rays(rays, unit=True).all()
    moved = sh.copy()
    moved["sphere_position"][4] += np.asarray((0.0, 5.0, 0.0), F)  # out of these rays' way
    t.update_scene(moved, tr, ma)
    occ = t.occluded_rays(rays, unit=True)
    assert np.array_equal(occ, cast_hit(t, rays)) and not occ.any()
    t.close()


@pytest.mark.parametrize("kind", ["sah", "median"])
def test_a_query_sees_the_device_refit(kind, T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    cam = CAMERAS["mesh_smooth"][0]
    t = handle(T, "mesh_smooth", kind, refit=True)
    ph = primary(oracle, "mesh_smooth", 0)[2]
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    ph2 = primary(oracle, "mesh_smooth", 0, shapes=moved)[2]
    # at the limits of the moved scene: exactly the new distance is visible, one ulp more is occluded -- on the rays whose
    # distance the move changed one of the two answers would be the other one in the old scene
    hit = np.isfinite(ph2["t"])
    t2 = ph2["t"][hit].astype(F)
    assert (ph["t"][hit] != ph2["t"][hit]).any()
    rays = R.rays(cam[3, :3], ph2["dir"][hit], t2)
    assert not t.occluded_rays(rays, unit=True).any()
    rays["tmax"] = np.nextafter(t2, F(np.inf))
    assert t.occluded_rays(rays, unit=True).all()
    assert np.array_equal(t.occluded_rays(cam[3, :3], ph2["dir"], unit=True), np.isfinite(ph2["t"]))
    t.close()


# ---- 9. group --------------------------------------------------------------------------------------------------------------------
def test_group_forms_give_the_single_handles_words(T, oracle):
    sh, tr, ma = scene("mesh_smooth")
    cam = CAMERAS["mesh_smooth"][1]
    _, _, ph = primary(oracle, "mesh_smooth", 1)
    t = handle(T, "mesh_smooth", "sah")
    g = T.TracerGroup(FW, FH, n_devices=2, devices=[0, 0], rows_per_block=1)
    g.set_acceleration(1)
    g.scene_data = R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    a, b = g.occluded_rays(cam[3, :3], ph["dir"], unit=True), t.occluded_rays(cam[3, :3], ph["dir"], unit=True)
    assert np.array_equal(O.words_of(a), O.words_of(b)) and np.array_equal(a, np.isfinite(ph["t"]))
    segs = O.random_segments()
    assert np.array_equal(g.segment_rays(segs).view(np.uint32), t.segment_rays(segs).view(np.uint32))
    for x, y in zip(g.occluded_segments(segs, with_invalid=True), t.occluded_segments(segs, with_invalid=True)):
        assert np.array_equal(O.words_of(x), O.words_of(y))
    g.close(), t.close()


# ---- 10. the headless route ------------------------------------------------------------------------------------------------------
def test_headless_line_of_sight_prints_what_python_answers(T, tmp_path):
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    segs, answers = O.sphere_segments()
    finite = [k for k in range(len(segs)) if np.isfinite(segs[k]["from"]).all() and np.isfinite(segs[k]["to"]).all() and np.isfinite(segs[k]["end_gap"])]
    prefix = str(tmp_path / "s")
    cmd = [exe, "--scene", "spheres", "--width", "16", "--height", "8", "--spp", "1", "--bounces", "1", "--frames", "1", "--dump", prefix]
    for k in finite:
        a, b = ",".join(repr(float(x)) for x in segs[k]["from"]), ",".join(repr(float(x)) for x in segs[k]["to"])
        cmd += ["--line-of-sight", f"{a}:{b}:{float(segs[k]['end_gap'])!r}"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("line of sight ")]
    assert len(lines) == len(finite), out
    dumped = (np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    t = handle(T, dumped)
    occ, inv = t.occluded_segments(segs[finite], with_invalid=True)
    want = ["invalid" if i else "occluded" if o else "visible" for o, i in zip(occ, inv)]
    assert [l.rsplit(": ", 1)[1] for l in lines] == want == [answers[k] for k in finite]
    assert {"visible", "occluded", "invalid"} <= set(want)
    assert "frame(s)" in out  # ... then it rendered as before
    t.close()
