"""GPU: the history clamp (srt_set_denoise_history_clamp). The bounds planes against their numpy restatement
(tests/history_clamp_ref.py), the whole clamping set-up against it under a moved camera and the moved-shape cases of
tests/motion_ref.py (with history illumination and demodulation on and off, a waving mesh, T > 1), that a frame after a moved
shape does clamp, that off means off, a device group against the single handle, and quality on the pixels whose lighting
changed while a sphere is dragged over a plane."""
import json

import numpy as np
import pytest

import denoise_ref as D
import history_clamp_ref as HC
import motion_ref as M
import spatial_variance_ref as SV
import temporal_cases as TC
import vertex_motion_ref as V
from conftest import bits_equal
from gpu_harness import T, cam_at, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S
from test_gpu_denoise_demod import check_filter

pytestmark = pytest.mark.gpu
SRT_ERR_INVALID, SRT_ERR_STATE = 1, 3
TP = dict(history_limit=32, normal_threshold=0.9, depth_threshold=0.05)
SHARP = dict(sigma_normal=32.0, sigma_depth=0.25, sigma_albedo=0.02)  # the other sigma set: narrower in depth and albedo, wider in the normal
SIGMAS = ("sigma_normal", "sigma_depth", "sigma_albedo")


def handle(T, sky, scn, w, h, gamma=1.0, K=0, tp=TP, accel=0, motion=False, vertex=False, illum=False, demod=False, group=0, cam=None, time=31, **dn):
    """a tracer over scn (a name of gpu_harness.scene or the arrays), 2 spp, the denoiser with K passes, temporal reprojection and
    the switches as given; group > 0: a TracerGroup of that many virtual devices"""
    shapes, tris, mats = scene(scn) if isinstance(scn, str) else scn
    dn = dict(iterations=K, **dn)
    if group:
        t = T.TracerGroup(w, h, n_devices=group, devices=[0] * group, rows_per_block=8)
        t.set_skybox(sky)
        t.set_acceleration(accel)
        t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera() if cam is None else cam, time=time)
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        t.set_denoise(**dn)
        t.set_denoise_temporal(**tp)
        t.scene = (shapes, tris, mats)
    else:
        t = make(T, sky, (shapes, tris, mats), w, h, spp=2, accel=accel, time=time, cam=cam, denoise=dn, temporal=tp, motion=motion or vertex)
        if vertex:
            t.set_denoise_vertex_motion(True)
    if demod:
        t.set_denoise_demodulation(True)
    if illum:
        t.set_denoise_history_illumination(True)
    if gamma:
        t.set_denoise_history_clamp(gamma)
    return t


def same_history(a, b):
    assert a["valid"] == b["valid"]
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(a[k], b[k]), k


def next_frame(t, cam, time, scn=None):
    """the front-end while something moves: clear, update_scene, a new camera, one dispatch"""
    t.clear_canvas()
    t.update_scene(*(t.scene if scn is None else scn))
    if cam is not None:
        t.options["camera_to_world"] = cam
    t.options["time"] = time
    return t.render(1).copy()


# ---- the switch's rules ----------------------------------------------------------------------------------------------------------
def test_state_rules(T, sky):
    lib = T.load_library()
    w, h = 48, 32
    t = make(T, sky, "spheres", w, h, denoise=dict(iterations=0))
    assert lib.srt_set_denoise_history_clamp(t._h, 1.0) == SRT_ERR_STATE  # temporal reprojection is off
    assert lib.srt_set_denoise_history_clamp(t._h, 0.0) == 0
    assert lib.srt_read_denoise_history_bounds(t._h, None, None) == SRT_ERR_STATE  # never ran
    t.set_denoise_temporal()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf"), 64.5, 1e30):
        assert lib.srt_set_denoise_history_clamp(t._h, bad) == SRT_ERR_INVALID, bad
    for good in (1e-6, 0.5, 64.0, -0.0, 0.0):
        assert lib.srt_set_denoise_history_clamp(t._h, good) == 0, good
    with pytest.raises(T.SrtError):
        t.set_denoise_history_clamp(65)
    t.set_denoise_history_clamp(1.0)
    t.render(1)
    assert not t.last_setup_history_clamp()  # no history yet: nothing new is launched
    assert lib.srt_read_denoise_history_bounds(t._h, None, None) == SRT_ERR_STATE
    t.clear_canvas()
    assert not t.last_setup_history_clamp()
    t.render(1)
    assert t.last_setup_history_clamp()
    assert t.read_denoise_history_bounds()["taps"].max() == 49
    t.clear_canvas()
    before = t.read_denoise_history()
    assert before["valid"]
    t.set_denoise_history_clamp(0)
    t.set_denoise_history_clamp(2.0)
    same_history(before, t.read_denoise_history())  # toggling clears nothing
    t.set_denoise_history_clamp(0)
    t.render(1)
    assert not t.last_setup_history_clamp()
    t.set_denoise_history_clamp(2.0)
    t.clear_canvas()  # the switch changed after the filter: the clear runs its own set-up, the variant the filter would run now
    assert t.last_setup_history_clamp()
    t.set_denoise_temporal(history_limit=16)  # another setting of the temporal stage: the switch stays
    t.render(1)
    assert t.last_setup_history_clamp()
    t.clear_canvas()
    t.set_denoise_temporal(False)  # turning temporal off turns it off
    t.set_denoise_temporal()
    t.render(1)
    t.clear_canvas()
    t.render(1)
    assert not t.last_setup_history_clamp()
    t.set_denoise_history_clamp(1.0)
    t.set_denoise(False)  # and so does turning the denoiser off
    t.set_denoise(iterations=0)
    t.set_denoise_temporal()
    t.render(1)
    t.clear_canvas()
    t.render(1)
    assert not t.last_setup_history_clamp()
    t.close()
    p = T.Tracer(w, h)
    p.set_partition(0, 2)
    assert lib.srt_set_denoise_history_clamp(p._h, 1.0) == SRT_ERR_STATE  # never on a partitioned handle
    p.close()
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=8)
    assert lib.srt_group_set_denoise_history_clamp(g._g, 1.0) == SRT_ERR_STATE  # no denoiser yet
    assert lib.srt_group_set_denoise_history_clamp(g._g, float("nan")) == SRT_ERR_INVALID
    assert lib.srt_group_set_denoise_history_clamp(g._g, 0.0) == 0
    assert not g.last_setup_history_clamp()
    g.close()


def test_the_history_does_not_depend_on_whether_a_filter_ran(T, sky):
    """trace alone, then clear: the clear's own set-up runs the bounds launch and the kernel the filter launches"""
    w, h = 64, 48
    a, b = (handle(T, sky, "spheres", w, h) for _ in range(2))
    for k in range(3):
        for t in (a, b):
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(k, "move")
            t.options["time"] = 40 + k
        a.render(1)
        b.trace()
        for t in (a, b):
            t.clear_canvas()
            assert t.last_setup_history_clamp() == (k > 0)
        same_history(a.read_denoise_history(), b.read_denoise_history())
    a.close()
    b.close()


# ---- 1. the bounds planes against the restatement ---------------------------------------------------------------------------------
BOUNDS_FRAMES = [(128, 72), (37, 29), (33, 7), (1, 33), (33, 1)]  # tiles cut by every border, a halo wider than the image


@pytest.mark.parametrize("scn,accel", [("spheres", 0), ("mixed", 1)])
@pytest.mark.parametrize("w,h", BOUNDS_FRAMES)
def test_bounds_planes_match_numpy(T, sky, w, h, scn, accel):
    """both sigma sets, T = 1 and T = 2. The tolerance is the spatial variance estimate's for its sums on the device
    (tests/test_gpu_denoise_spatial_variance.py: rtol 1e-3, atol 1e-9 on a variance), here on mu, the sum of weights and
    sigma^2; the tap counts and the pixels that do not clamp are equal exactly."""
    t = handle(T, sky, scn, w, h, accel=accel, cam=cam_at(0, "move"))
    t.render(1)
    pixels = 0
    for T_ in (1, 2):
        t.clear_canvas()
        t.update_scene(*t.scene)
        t.options["camera_to_world"] = cam_at(2 + T_, "move")
        for d in range(T_):
            t.options["time"] = 2001 + 10 * T_ + d
            t.render(d + 1)
        inp = t.read_denoise_inputs()
        assert inp["T"] == T_
        cur = HC.TR.frame(t.read_canvas(), inp, inp["T"])
        for sig in ({}, SHARP):
            t.set_denoise(iterations=0, **sig)
            t.resolve_denoised(T_)
            assert t.last_setup_history_clamp()
            got, want = t.read_denoise_history_bounds(), HC.bounds(cur, **sig)
            what = f"{scn} {w}x{h} T={T_} {sig}"
            assert np.array_equal(got["taps"], want["taps"].astype(np.float32)), what
            assert np.array_equal(got["weight"] > 0, want["weight"] > 0), what
            np.testing.assert_allclose(got["weight"], want["weight"], rtol=1e-3, atol=1e-9, err_msg=what)
            np.testing.assert_allclose(got["mu"], want["mu"], rtol=1e-3, atol=1e-9, err_msg=what)
            np.testing.assert_allclose(got["sigma"] * got["sigma"], want["sigma"] * want["sigma"], rtol=1e-3, atol=1e-9, err_msg=what)
            pixels += int((want["weight"] > 0).sum())
        t.set_denoise(iterations=0)
    assert pixels > 0
    t.close()


# ---- 2., 3. the whole set-up against the restatement --------------------------------------------------------------------------------
def check_setup(t, want, argb, label, got=None, exact_bits=True):
    """§11's rule (tests/temporal_cases.py compare_setup) with the clamp's exemption: the frame just rendered (K = 0) and the
    history the clear commits against want = history_clamp_ref.temporal_setup(). Pixels the restatement does not clamp: bit for
    bit off the flagged ones (exact_bits False: rtol 1e-4, the per-triangle map's rule) -- and so bit for bit the restatement's
    switch-off set-up. Clamped pixels: rtol 1e-4 and bytes within 1. Flagged pixels (the reprojection's own flags, or a history colour
    within rtol 1e-4 of a bound) are exempt where they differ; at most 1 % of a frame may be flagged. -> the committed history"""
    w, h = t.width, t.height
    got = t.read_denoised() if got is None else got
    t.clear_canvas()
    assert t.last_setup_history_clamp()
    got_h = t.read_denoise_history()
    assert got_h["valid"]
    exact, close, worst = TC.compare_setup(want, got, argb.reshape(h, w, 4), got_h)
    border, clamped = want["rep"]["borderline"], want["rep"]["clamped"]
    print(f"{label} {w}x{h}: {int(clamped.sum())} pixels clamped, {int(border.sum())} flagged ({int(want['rep']['near_edge'].sum())} near a bound), "
          f"{int((~exact).sum())} differ in a bit ({int((~exact & ~border & ~clamped).sum())} unflagged and unclamped), {int((~close).sum())} beyond rtol 1e-4")
    assert border.mean() <= 0.01, label
    bad = ~(exact if exact_bits else close) & ~border & ~clamped
    assert not bad.any(), (label, np.argwhere(bad)[:5])
    assert not (~close & ~border).any(), (label, np.argwhere(~close & ~border)[:5])
    return got_h


@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("gamma", [1.0, 4.0])
def test_dolly_matches_numpy(T, sky, gamma, illum):
    """four 2-spp frames along the `dolly` case of tests/temporal_cases.py over the mixed scene (BVH); the second and fourth frame
    are two dispatches (T = 2)"""
    w, h = 128, 72
    t = handle(T, sky, "mixed", w, h, gamma=gamma, accel=1, illum=illum)
    clamped = 0
    for k in range(5):
        m, fov, _ = TC.interpolate("dolly", k, 4)
        t.clear_canvas()
        hist = t.read_denoise_history()
        t.update_scene(*t.scene)
        t.options["camera_to_world"], t.options["fov_scale"] = m, fov
        for d in range(2 if k in (2, 4) else 1):
            t.options["time"] = 3000 + 10 * k + d
            argb = t.render(d + 1).copy()
        if k == 0:
            assert not t.last_setup_history_clamp()
            continue
        inp = t.read_denoise_inputs()
        want = HC.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, gamma, rescale=illum, **TP)
        assert t.last_setup_history_illumination() == illum
        check_setup(t, want, argb, f"dolly frame {k} gamma {gamma} illum {illum}")  # (it clears: the loop's own clear then commits nothing new)
        clamped += int(want["rep"]["clamped"].sum())
    assert clamped > 0
    t.close()


@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("case", M.MOVES, ids=[m[0] for m in M.MOVES])
def test_moved_shapes_match_numpy(T, sky, case, illum, demod):
    """the moved-shape cases of tests/motion_ref.py at gamma 1 and 4. Without demodulation K = 0: colour, variance, bytes and the
    committed history. With it K = 1 (demodulation acts on K >= 1): the set-up still outputs colour, so the committed history is
    held the same way and the filtered frame to §10's tolerances over the restatement's set-up. A frame after a moved shape must
    clamp more than 1 % of its pixels -- by the restatement, so the test cannot pass by never clamping."""
    name, scn_name, accel, cam_kind, steps = case
    w, h = M.SIZE
    shapes, tris, mats = scene(scn_name)
    for gamma in (1.0, 4.0):
        t = handle(T, sky, (shapes, tris, mats), w, h, gamma=gamma, K=1 if demod else 0, accel=accel, motion=True, illum=illum, demod=demod,
                   cam=cam_at(0, cam_kind))
        t.render(1)
        most = 0.0
        for k in range(1, M.FRAMES):
            t.clear_canvas()
            hist = t.read_denoise_history()
            hist["ids"] = t.read_denoise_shape_ids()[1]
            now = M.move_shapes(shapes, tris, steps, k)
            t.update_scene(now, tris, mats)
            table = t.read_denoise_motion()
            assert t.read_denoise_history()["valid"] and table["any_moved"]
            t.options["camera_to_world"] = cam_at(k, cam_kind)
            t.options["time"] = 2000 + k
            argb = t.render(1).copy().reshape(h, w, 4)
            assert t.last_setup_history_clamp() and t.last_filter_demodulated() == demod
            inp = t.read_denoise_inputs()
            ids = t.read_denoise_shape_ids()[0]
            want = HC.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, gamma, ids=ids, table=table, rescale=illum, **TP)
            label = f"{name} frame {k} gamma {gamma} illum {illum} demod {demod}"
            border, clamped = want["rep"]["borderline"], want["rep"]["clamped"]
            if not demod:
                check_setup(t, want, argb, label)
            else:
                got = t.read_denoised()
                t.clear_canvas()
                got_h = t.read_denoise_history()
                dummy = np.concatenate([want["c"], want["V"][..., None]], -1)
                exact, close, _ = TC.compare_setup(want, dummy, D.tonemap(want["c"]), got_h)  # the committed history alone
                assert border.mean() <= 0.01, label
                assert not (~exact & ~border & ~clamped).any() and not (~close & ~border).any(), label
                if not (~exact & border).any():  # (a flagged pixel decided the other way feeds its neighbours in the pass)
                    cur = want["cur"]
                    st, _ = SV.filter_steps(want["c"], want["V"], cur["N"], cur["Z"], cur["A"], cur["cov"], None, None, None, 0, iterations=1, demod=True)
                    check_filter(got, argb, *st[1], label)
            t.update_scene(now, tris, mats)
            most = max(most, float(clamped.mean()))
        print(f"{name} gamma {gamma} illum {illum} demod {demod}: at most {most * 100:.1f} % of a frame clamped")
        if gamma == 1.0:
            assert most > 0.01, name
        t.close()


def test_waving_mesh_matches_numpy(T, sky):
    """the deform kernel's clamping form, with and without history illumination; §17's comparison (rtol 1e-4 off the flagged pixels)"""
    w, h = 64, 48
    for illum in (False, True):
        t = handle(T, sky, "meshes", w, h, accel=1, vertex=True, illum=illum)
        shapes, tris, mats = t.scene
        t.render(1)
        t.clear_canvas()
        hist = t.read_denoise_history()
        hist["ids"] = t.read_denoise_shape_ids()[1]
        h_rows = t.read_denoise_vertex_tables()[1]
        now = V.wave(tris, 12, 968, 1, 0.02)
        t.update_scene(shapes, now, mats)
        table = t.read_denoise_motion()
        want_table = V.scene_table((shapes, tris, mats, t.scene_data), (shapes, now, mats, t.scene_data))
        assert t.read_denoise_history()["valid"] and table["any_moved"] and (want_table["state"] == V.DEFORMED).any()
        table["first_row"] = want_table["first_row"]
        t.options["time"] = 2001
        argb = t.render(1).copy()
        ids, tri_ids = t.read_denoise_shape_ids()[0], t.read_denoise_triangle_ids()[0]
        rows = t.read_denoise_vertex_tables()[0]
        inp = t.read_denoise_inputs()
        want = HC.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, 1.0, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows,
                                 rescale=illum, **TP)
        check_setup(t, want, argb, f"a waving mesh illum {illum}", exact_bits=False)
        on = want["rep"]["state"] == V.DEFORMED
        assert (on & (want["h"] > 0)).any() and want["rep"]["clamped"].any()
        t.close()


def test_spatial_variance_reads_what_the_clamping_setup_staged(T, sky):
    """§18 over the clamping set-up: the staged count and moments are the restatement's, and the filtered frame is §18's
    restatement over them"""
    from test_gpu_denoise_spatial_variance import adopt_staged
    w, h, K, ms = 64, 48, 5, 8
    t = handle(T, sky, "spheres", w, h, K=K, cam=cam_at(0, "move"))
    t.set_denoise_spatial_variance(ms)
    t.render(1)
    t.clear_canvas()
    hist = t.read_denoise_history()
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam_at(3, "move")
    t.options["time"] = 2001
    argb = t.render(1).copy().reshape(h, w, 4)
    assert t.last_setup_history_clamp() and t.last_filter_spatial_variance()
    got = t.read_denoised()
    inp = t.read_denoise_inputs()
    want = HC.temporal_setup(t.read_canvas(), inp, inp["T"], hist, t.options, 1.0, **TP)
    cur = want["cur"]
    st = dict(c=want["c"], V=want["V"], N=cur["N"], Z=cur["Z"], A=cur["A"], cov=cur["cov"], src=SV.sources_staged(want["commit"]),
              commit=want["commit"], borderline=want["rep"]["borderline"] | want["rep"]["clamped"])
    t.clear_canvas()
    adopt_staged(st, t.read_denoise_history())  # (flagged and clamped pixels: the library's staged values, equal within rtol 1e-4)
    steps, _ = SV.filter_steps(st["c"], st["V"], st["N"], st["Z"], st["A"], st["cov"], *st["src"], ms, iterations=K)
    check_filter(got, argb, *steps[K], "spatial variance over the clamping set-up")
    assert want["rep"]["clamped"].mean() > 0.01
    t.close()


# ---- 4. off means off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [False, True])
def test_off_means_off(T, sky, motion):
    """a handle that never called the switch, one that turned it on and off again before the sequence, and one that has it on:
    the first two give the same bits (the parent's kernels: profiles/r20_history_clamp_isa_compare.txt) in every output over the
    sequence, the third does not"""
    w, h = 64, 48
    shapes, tris, mats = scene("spheres")
    steps = [(4, "translate", (0.05, 0.02, 0.03))]
    never = handle(T, sky, "spheres", w, h, gamma=0, K=2, motion=motion)
    off = handle(T, sky, "spheres", w, h, gamma=2.0, K=2, motion=motion)
    on = handle(T, sky, "spheres", w, h, gamma=1.0, K=2, motion=motion)
    off.set_denoise_history_clamp(0)
    differ = False
    for k in range(4):
        scn = (M.move_shapes(shapes, tris, steps, k), tris, mats) if motion else None
        outs = [next_frame(t, None if motion else cam_at(k, "move"), 600 + k, scn) for t in (never, off, on)]
        assert not never.last_setup_history_clamp() and not off.last_setup_history_clamp() and on.last_setup_history_clamp() == (k > 0)
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(never.read_denoised(), off.read_denoised()), k
        differ |= not np.array_equal(outs[0], outs[2])
    for t in (never, off, on):
        t.clear_canvas()
    same_history(never.read_denoise_history(), off.read_denoise_history())
    assert never.read_denoise_history()["valid"] and differ
    for t in (never, off, on):
        t.close()


# ---- 5. a device group -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_handle(T, sky, n):
    w, h = 48, 40
    single, group = (handle(T, sky, "spheres", w, h, K=2, illum=True, group=g) for g in (0, n))
    for k in range(4):
        outs = []
        for t in (single, group):
            outs.append(next_frame(t, cam_at(k, "yaw"), 500 + k))
            assert t.last_setup_history_clamp() == (k > 0)
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(single.read_denoised(), group.read_denoised()), k
    for t in (single, group):
        t.clear_canvas()
    same_history(single.read_denoise_history(), group.read_denoise_history())
    for t in (single, group):
        t.set_denoise_history_clamp(0)
    assert np.array_equal(single.render(1), group.render(1)) and not group.last_setup_history_clamp()
    group.set_denoise_temporal(False)
    assert T.load_library().srt_group_set_denoise_history_clamp(group._g, 1.0) == SRT_ERR_STATE  # the group's temporal reprojection is off
    single.close()
    group.close()


# ---- 6. quality on the pixels whose lighting changed --------------------------------------------------------------------------------
GAMMAS = (0.5, 1.0, 2.0, 4.0)
# Measured on an MI355X (profiles/r20_history_clamp_quality.json; runs are bit-identical). Per gamma: the ratio of the tonemapped
# MSE with the clamp on over the clamp off, on the stale set and on the whole frame. None: not measured yet.
MEASURED = {0.5: dict(stale_ratio=1.2386, frame_ratio=2.0983), 1.0: dict(stale_ratio=1.1788, frame_ratio=1.8504),
            2.0: dict(stale_ratio=1.1098, frame_ratio=1.5912), 4.0: dict(stale_ratio=1.0570, frame_ratio=1.3528)}
# No gamma brings the stale-set ratio below 1 (127 stale pixels; clamp off 8.310e-3 on them, 2.197e-3 over the frame): at 2 spp the
# 7x7 neighbourhood's own mean is noisier than the history it corrects, so the clamp costs more everywhere than it wins where the
# lighting changed. No quality claim is made; the library ships gamma = 1 as its advice, and this test only
# holds the whole-frame ratio at that gamma under the measured value plus 0.1.
SHIPPED_GAMMA = 1.0


def drag_scene(x):
    """a diffuse sphere above a diffuse floor under the sun; x: the sphere's place along its drag"""
    shapes, mats = np.zeros(2, R.SHAPE), np.zeros(2, R.MATERIAL)
    shapes[0], shapes[1] = R.plane(0, (0, -1, 0), (0, 1, 0)), R.sphere(1, (x, 0.2, -1.5), 0.9)
    mats[0], mats[1] = R.material((0.8, 0.8, 0.8)), R.material((0.9, 0.35, 0.3))
    return shapes, R.box_triangles(), mats


def drag_handle(T, sky, x, spp=2, gamma=0.0, **kw):
    t = make(T, sky, drag_scene(x), 160, 90, spp=spp, time=4242, **kw)
    t.scene_data = R.scene_data(2, sun_focus=200.0, sun_intensity=20.0)
    t.update_scene(*t.scene)
    t.clear_canvas()
    if gamma:
        t.set_denoise_history_clamp(gamma)
    return t


def test_quality_stale_lighting(T, sky):
    """160x90, 2 spp, default filter, object motion on, the sphere dragged along x for 8 frames; 4096 spp references at the first and
    the last pose. The stale set: the same first-hit shape in both references, not the moved shape, tonemapped references that
    differ by more than 0.05 in a channel. The eighth frame against the last-pose reference, clamp on over clamp off."""
    frames, xs = 8, [-1.2 + 0.3 * k for k in range(8)]
    refs, ids = [], []
    for x in (xs[0], xs[-1]):
        g = drag_handle(T, sky, x, spp=4096, denoise=dict(iterations=0), temporal={}, motion=True)
        g.render(1)
        refs.append(tone(g.read_canvas()[..., :3]))
        ids.append(g.read_denoise_shape_ids()[0])
        g.close()
    stale = (ids[0] == ids[1]) & (ids[1] != 1) & (ids[0] != 1) & (np.abs(refs[0] - refs[1]).max(-1) > 0.05)
    assert stale.sum() > 0
    ref = refs[1]
    runs = {g: drag_handle(T, sky, xs[0], gamma=g, denoise={}, temporal={}, motion=True) for g in (0.0,) + GAMMAS}
    for k in range(frames):
        for g, t in runs.items():
            next_frame(t, None, 900 + k, drag_scene(xs[k]))
            assert t.read_denoise_history()["valid"] == (k > 0) and t.last_setup_history_clamp() == (k > 0 and g > 0)
    out = {g: t.read_denoised()[..., :3] for g, t in runs.items()}
    for t in runs.values():
        t.close()
    mse = lambda x, m=slice(None): float(np.mean((tone(x)[m] - ref[m]) ** 2))
    record = {"frame": [160, 90], "spp": 2, "frames": frames, "stale_pixels": int(stale.sum()), "off": {"stale": mse(out[0.0], stale), "frame": mse(out[0.0])}}
    for g in GAMMAS:
        record[str(g)] = {"stale": mse(out[g], stale), "frame": mse(out[g]), "stale_ratio": mse(out[g], stale) / mse(out[0.0], stale),
                          "frame_ratio": mse(out[g]) / mse(out[0.0])}
    print("history clamp quality: " + json.dumps(record))
    got = record[str(SHIPPED_GAMMA)]
    assert not bits_equal(out[SHIPPED_GAMMA], out[0.0])  # (a clamp that does nothing would give the clamp-off frame)
    assert all(m["stale_ratio"] >= 1.0 for m in MEASURED.values())  # the null result this test was written under
    assert got["frame_ratio"] <= MEASURED[SHIPPED_GAMMA]["frame_ratio"] + 0.1


# ---- srt_headless ------------------------------------------------------------------------------------------------------------------
def test_headless_history_clamp_writes_another_frame(tmp_path):
    """srt_headless --denoise 5 --temporal --move-shape --history-clamp: a frame comes out, and it is not the frame without the switch"""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    frames = []
    for extra in ([], ["--history-clamp", "1"]):
        out = tmp_path / f"f{len(extra)}.ppm"
        subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", "3", "--denoise", "5", "--temporal",
                        "--move-shape", "4", "0.05", "--out", str(out)] + extra, check=True, timeout=120)
        frames.append(out.read_bytes())
    assert frames[1].startswith(b"P6") and len(frames[0]) == len(frames[1]) > 64 * 48 * 3
    assert frames[0] != frames[1]
