"""CPU: the history clamp's restatement (tests/history_clamp_ref.py; include/srt_abi.h srt_set_denoise_history_clamp) on analytic
inputs, the symbols and their NULL arguments, srt_headless's usage rule, and the share of pixels the restatement flags on
frames of the GPU test's scenes and moves (tests/test_gpu_denoise_history_clamp.py)."""
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as D
import history_clamp_ref as HC
import motion_ref as M
import temporal_cases as TC
import temporal_ref as TR
from gpu_harness import cam_at, scene
from simple_raytracer_amd import records as R

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
SRT_ERR_INVALID = 1
CALLS = ["srt_set_denoise_history_clamp", "srt_group_set_denoise_history_clamp", "srt_last_setup_history_clamp",
         "srt_group_last_setup_history_clamp", "srt_read_denoise_history_bounds"]
W, H = 24, 16


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def test_symbols_and_null_arguments(T):
    """gamma's validation needs a handle, and a handle needs a device: the GPU test holds it (test_state_rules); here the calls
    exist, are declared, are bound, and answer a NULL handle"""
    lib = T.load_library()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include/srt_abi.h").read_text(), flags=re.S)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in T.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for g in (0.0, 1.0, -1.0, float("nan")):
        assert lib.srt_set_denoise_history_clamp(None, g) == SRT_ERR_INVALID
        assert lib.srt_group_set_denoise_history_clamp(None, g) == SRT_ERR_INVALID
    assert lib.srt_last_setup_history_clamp(None) == 0 and lib.srt_group_last_setup_history_clamp(None) == 0
    assert lib.srt_read_denoise_history_bounds(None, None, None) == SRT_ERR_INVALID
    for method in ("set_denoise_history_clamp", "last_setup_history_clamp"):
        assert getattr(T.TracerGroup, method) is getattr(T.Tracer, method)


def test_headless_history_clamp_needs_temporal(T):
    """srt_headless --history-clamp G without --denoise K --temporal is a usage error, before any device is touched"""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    for args in (["--history-clamp", "1"], ["--denoise", "5", "--history-clamp", "1"]):
        r = subprocess.run([str(exe), "--scene", "spheres"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--history-clamp G needs --denoise K --temporal" in r.stderr
    r = subprocess.run([str(exe), "--scene", "spheres", "--denoise", "5", "--temporal", "--history-clamp", "-2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--history-clamp G needs" in r.stderr


# ---- analytic frames -----------------------------------------------------------------------------------------------------------
def flat(colour=(0.5, 0.25, 0.75), P=2):
    """a wall facing the camera at depth 5, one albedo, one colour: a frame of temporal_ref (the default colour's sums over 49
    taps of weight 1 are exact in float32, so mu is the colour and sigma is 0 to the bit)"""
    c = np.ones((H, W, 3), F32) * F32(colour)
    N = np.zeros((H, W, 3), F32)
    N[..., 2] = 1
    m1 = D.lum(c)
    return dict(c=c, m1=m1, m2=(m1 * m1).astype(F32), V=np.zeros((H, W), F32), N=N, Z=np.full((H, W), F32(5)), A=np.full((H, W, 3), F32(0.7)),
                cov=np.ones((H, W), F32), P=P)


def rep_of(colour, m1=None, m2=None, count=6.0):
    """a reprojection that found history everywhere"""
    c = (np.ones((H, W, 3), F32) * np.asarray(colour, F32)).astype(F32)
    m1 = D.lum(c) if m1 is None else np.full((H, W), F32(m1))
    m2 = (m1 * m1 + F32(0.04)).astype(F32) if m2 is None else np.full((H, W), F32(m2))
    return dict(h=np.full((H, W), F32(count)), c=c, m1=m1, m2=m2, taps=np.ones((H, W), np.int32), borderline=np.zeros((H, W), bool))


def noisy(seed=3):
    cur = flat()
    cur["c"] = np.random.default_rng(seed).uniform(0.2, 0.8, (H, W, 3)).astype(F32)
    cur["m1"] = D.lum(cur["c"])
    return cur


def test_flat_neighbourhood_pulls_any_history_exactly_to_the_mean():
    cur = flat()
    b = HC.bounds(cur)
    assert np.all(b["sigma"] == 0) and np.all(b["weight"] > 0) and TC.same_bits(b["mu"], cur["c"]).all()
    assert b["taps"].max() == 49 and b["taps"][0, 0] == 16 and b["taps"][0, 3] == 28  # the corner's 4x4, an edge's 4x7
    for gamma in (0.5, 4.0, 64.0):
        for x in ((3.0, 0.0, 0.3), (0.0, 9.0, 1e-3), (1e30, 0.4, -1.0)):
            out = HC.clamp(rep_of(x), b, gamma)
            assert out["clamped"].all() and TC.same_bits(out["c"], cur["c"]).all()
            assert TC.same_bits(out["m1"][None], D.lum(cur["c"])[None]).all()


def test_history_inside_the_box_changes_nothing():
    """every output of the set-up is temporal_ref's, bit for bit, and the moments are not touched"""
    cur = noisy()
    b = HC.bounds(cur)
    assert np.all(b["sigma"] > 0.05)
    rep = rep_of((0.5, 0.5, 0.5))
    lo, hi = b["mu"] - F32(4) * b["sigma"], b["mu"] + F32(4) * b["sigma"]
    assert np.all((rep["c"] > lo) & (rep["c"] < hi))
    out = HC.clamp(rep, b, 4.0)
    assert not out["clamped"].any()
    for k in ("c", "m1", "m2", "h"):
        assert TC.same_bits(np.atleast_3d(out[k]), np.atleast_3d(rep[k])).all(), k
    want, got = TR.integrate(cur, rep), TR.integrate(cur, out)
    for k in ("c", "V"):
        assert TC.same_bits(np.atleast_3d(got[k]), np.atleast_3d(want[k])).all(), k
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert TC.same_bits(np.atleast_3d(got["commit"][k]), np.atleast_3d(want["commit"][k])).all(), k
    # a tighter gamma on the same frame does clamp: the test above is not vacuous
    assert HC.clamp(rep, b, 0.5)["clamped"].any()


@pytest.mark.parametrize("edge", ["normal", "depth", "albedo"])
def test_taps_across_an_edge_do_not_widen_the_box(edge):
    """left half dark, right half bright, and between them a geometric edge: a pixel beside the edge keeps the box of its own
    side (without the edge the box spans both)"""
    cur = flat((0.2, 0.2, 0.2))
    cur["c"][:, W // 2:] = F32(5.0)
    plain = HC.bounds(cur)
    x = W // 2 - 1
    assert plain["sigma"][H // 2, x, 0] > 1.0  # no edge: both sides weigh in
    if edge == "normal":
        cur["N"][:, W // 2:] = F32([1, 0, 0])
    elif edge == "depth":
        cur["Z"][:, W // 2:] = F32(5000)
    else:
        cur["A"][:, W // 2:] = F32(0.1)
    b = HC.bounds(cur)
    assert b["taps"][H // 2, x] == 49  # they count, and weigh nothing (or next to it)
    assert b["sigma"][H // 2, x].max() < 1e-3 and abs(b["mu"][H // 2, x, 0] - 0.2) < 1e-3
    out = HC.clamp(rep_of((5.0, 5.0, 5.0)), b, 1.0)
    assert out["clamped"][H // 2, x] and abs(out["c"][H // 2, x, 0] - 0.2) < 2e-3
    if edge != "depth":  # (the depth term is relative to the pixel's own depth: from the far side the near one is not far)
        assert b["sigma"][H // 2, x + 1].max() < 1e-3 and abs(b["mu"][H // 2, x + 1, 0] - 5.0) < 1e-2 and not out["clamped"][H // 2, x + 1]


def test_four_counting_taps_give_no_clamp_and_five_do():
    cur = flat()
    cur["cov"][:] = 0
    cur["cov"][8, 8:12] = 1  # a line of 4: each pixel counts 4 taps
    cur["cov"][2, 2:7] = 1   # a line of 5: its middle pixel counts all 5, its ends 4
    b = HC.bounds(cur)
    assert np.all(b["taps"][8, 8:12] == 4) and np.all(b["weight"][8, 8:12] == 0) and np.all(b["sum_w"][8, 8:12] > 0)
    assert b["taps"][2, 2:7].tolist() == [4, 5, 5, 5, 4] and np.all(b["weight"][2, 3:6] > 0) and b["weight"][2, 2] == 0
    assert b["taps"][0, 0] == 0 and b["weight"][0, 0] == 0 and not b["mu"][0, 0].any()  # a pixel that does not qualify: zeros
    out = HC.clamp(rep_of((9.0, 9.0, 9.0)), b, 1.0)
    assert not out["clamped"][8, 8:12].any() and out["clamped"][2, 3:6].all() and not out["clamped"][2, 2]
    assert TC.same_bits(out["c"][8:9, 8:12], np.full((1, 4, 3), F32(9))).all()


def test_nan_inf_and_zero_coverage_taps_are_ignored():
    cur = flat()
    clean = HC.bounds(cur)
    cur["c"][5, 5] = (np.nan, 0.25, 0.75)
    cur["c"][5, 7] = (0.5, np.inf, 0.75)
    cur["c"][6, 6] = (100.0, 100.0, 100.0)
    cur["cov"][6, 6] = 0
    b = HC.bounds(cur)
    assert b["taps"][5, 6] == 49 - 3 and b["taps"][5, 5] == 0 and b["weight"][5, 5] == 0 and b["weight"][6, 6] == 0
    near = np.zeros((H, W), bool)
    near[2:10, 2:11] = True
    ok = near & (b["taps"] > 0)
    assert TC.same_bits(b["mu"][ok][None], clean["mu"][ok][None]).all() and np.all(b["sigma"][ok] == 0) and np.all(np.isfinite(b["mu"]))
    # a spread whose square overflows: no range, so no clamp
    cur = flat()
    cur["c"][::2, :, 0] = F32(1e30)  # every neighbourhood spans 1e30: the squared difference is not finite
    assert np.all(HC.bounds(cur)["weight"] == 0)
    # a NaN in the history colour moves nothing (and is no clamped pixel)
    rep = rep_of((np.nan, 9.0, 9.0))
    out = HC.clamp(rep, clean, 1.0)
    assert np.isnan(out["c"][..., 0]).all() and np.all(out["c"][..., 1] == clean["mu"][..., 1])


def test_moments_follow_the_colour_and_keep_their_variance():
    cur = flat()
    b = HC.bounds(cur)
    rep = rep_of((2.0, 2.0, 2.0), m1=2.0, m2=4.25)
    out = HC.clamp(rep, b, 1.0)
    m1 = D.lum(cur["c"])
    assert out["clamped"].all() and TC.same_bits(out["m1"][None], m1[None]).all()
    np.testing.assert_allclose(out["m2"] - out["m1"] * out["m1"], 0.25, rtol=1e-5)
    # a history whose m2 is below m1^2 (rounding) keeps a variance of 0, not a negative one
    out = HC.clamp(rep_of((2.0, 2.0, 2.0), m1=2.0, m2=3.9), b, 1.0)
    assert TC.same_bits(out["m2"][None], (m1 * m1).astype(F32)[None]).all()


def test_no_history_and_gamma_zero_run_no_clamp():
    cur_rd = R.render_data(W, H, 2, 10)
    canvas = np.random.default_rng(1).uniform(0.1, 1.0, (H, W, 4)).astype(F32)
    inputs = dict(normal_depth=np.tile(F32([0, 0, 1, 5]), (H, W, 1)), albedo_hits=np.tile(F32([0.7, 0.7, 0.7, 1]), (H, W, 1)),
                  moments=np.ones((H, W), F32), T=1, P=2)
    out = HC.temporal_setup(canvas, inputs, 1, dict(valid=False), cur_rd, 1.0)
    assert out["bounds"] is None and not out["rep"]["clamped"].any()
    hist = TR.history_from_commit(out["commit"], cur_rd)
    hist["colour"] = (hist["colour"] + F32(3)).astype(F32)
    assert HC.temporal_setup(canvas, inputs, 1, hist, cur_rd, 0.0)["bounds"] is None
    on = HC.temporal_setup(canvas, inputs, 1, hist, cur_rd, 1.0)
    assert on["rep"]["clamped"].mean() > 0.9 and not TC.same_bits(on["c"], on["off"]["c"]).all()


# ---- the flagged share on frames of the GPU test's scenes ----------------------------------------------------------------------
def oracle_frame(oracle, sky, arrays, rdata):
    """a 2-spp frame of the oracle as temporal_ref.frame(): its canvas, its feature pass, moments to match"""
    shapes, tris, mats = arrays
    sd = R.scene_data(len(shapes))
    canvas = oracle.render(rdata, sd, shapes, tris, mats, sky)
    nd, ah = oracle.features(rdata, sd, shapes, tris, mats, 1)
    lum = D.lum(canvas[..., :3])
    inputs = dict(normal_depth=nd, albedo_hits=ah, moments=(F32(1.5) * lum * lum).astype(F32), T=1, P=2)
    return canvas, inputs


@pytest.mark.parametrize("gamma", [1.0, 4.0])
@pytest.mark.parametrize("case", ["dolly"] + [m[0] for m in M.MOVES])
def test_restatement_flags_under_a_hundredth_of_a_frame(oracle, sky, case, gamma):
    """The GPU test's cap is 1 % of a frame flagged (the reprojection's own flags and a history colour within rtol 1e-4 of a bound).
    Here the restatement alone, on the oracle's 2-spp frames of the same scenes under the same moves (frame 0 commits, frame 1
    is set up; the GPU test asserts the cap again on every frame it renders): the device's samples differ, the geometry does
    not."""
    w, h = M.SIZE
    if case == "dolly":
        arrays = scene("mixed")
        frames = [(arrays, TC.render_record(w, h, cam, time=2000 + k)) for k, cam in enumerate(TC.CASES["dolly"])]
    else:
        _, scn_name, _, cam_kind, steps = next(m for m in M.MOVES if m[0] == case)
        shapes, tris, mats = scene(scn_name)
        frames = [((M.move_shapes(shapes, tris, steps, k), tris, mats), R.render_data(w, h, 2, 10, camera_to_world=cam_at(k, cam_kind), time=2000 + k))
                  for k in range(2)]
    (a0, rd0), (a1, rd1) = frames
    canvas, inputs = oracle_frame(oracle, sky, a0, rd0)
    first = HC.temporal_setup(canvas, inputs, 1, dict(valid=False), rd0, gamma)
    hist = TR.history_from_commit(first["commit"], rd0)
    ids = table = None
    if case != "dolly":
        sd = R.scene_data(len(a0[0]))
        hist["ids"] = TC.features_frame(oracle, rd0, *a0)[1]
        ids = TC.features_frame(oracle, rd1, *a1)[1]
        table = M.scene_table((*a0, sd), (*a1, sd))
    canvas, inputs = oracle_frame(oracle, sky, a1, rd1)
    out = HC.temporal_setup(canvas, inputs, 1, hist, rd1, gamma, ids=ids, table=table)
    flagged, clamped = out["rep"]["borderline"].mean(), out["rep"]["clamped"].mean()
    print(f"{case} gamma {gamma}: {flagged * 100:.3f} % flagged ({out['rep']['near_edge'].sum()} near a bound), {clamped * 100:.1f} % clamped")
    assert flagged <= 0.01 and (out["h"] > 0).mean() > 0.2
