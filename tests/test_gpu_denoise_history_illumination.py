"""GPU: the history reprojected as illumination (srt_set_denoise_history_illumination). The switch's rules, a
still camera and a one-colour scene bit for bit against the switch off, the three illumination kernels against their numpy
restatement (tests/history_illumination_ref.py) under a moved camera, a moved sphere and a waving mesh, the filter with
demodulation and the spatial variance estimate on top of the new set-up, a device group against the single handle, and quality:
on the noise-textured scene against the switch off (the parent's behaviour), on untextured scenes against §11's thresholds."""
import numpy as np
import pytest

import history_illumination_ref as HI
import motion_ref as M
import spatial_variance_ref as SV
import temporal_cases as TC
import vertex_motion_ref as V
from conftest import bits_equal
from gpu_harness import T, cam_at, make, scene, tone  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S
from test_gpu_denoise_demod import check_filter
from test_gpu_denoise_spatial_variance import adopt_staged

pytestmark = pytest.mark.gpu
SRT_ERR_STATE = 3
TP = dict(history_limit=32, normal_threshold=0.9, depth_threshold=0.05)
FS = 2  # feature_samples = num_samples on textured scenes (the guide's texel is then the canvas's)


def case(kind):
    """-> shapes, tris, mats, textures, bindings, uvs, accel"""
    if kind == "noise":
        return (*S.textured_noise_scene(), None, 0)
    if kind == "spheres":
        return (*S.textured_sphere_scene(), None, 0)
    if kind == "mesh":  # every material textured, planar UVs, under the BVH
        return (*S.textured_mesh_scene(), 1)
    if kind == "one-colour":  # the sphere scene, every material's colour the same: D_p and D_h are bit-equal wherever both are covered
        shapes, tris, mats = scene("spheres")
        mats = mats.copy()
        mats["color"][:, :3] = (0.7, 0.45, 0.3)
        return shapes, tris, mats, None, None, None, 0
    return (*scene(kind), None, None, None, 1 if kind == "meshes" else 0)  # untextured: gpu_harness.scene


def handle(T, sky, kind, w, h, K=0, tp=TP, illum=True, motion=False, vertex=False, demod=False, group=0, cam=None, time=31, **dn):
    """a tracer over case(kind) with its textures bound, 2 spp and 2 feature samples, the denoiser with K passes, temporal
    reprojection and the switch as given; group > 0: a TracerGroup of that many virtual devices"""
    shapes, tris, mats, textures, bindings, uvs, accel = case(kind)
    dn = dict(iterations=K, feature_samples=FS, **dn)
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
    if textures is not None:
        t.set_textures(textures)
        t.set_material_textures(bindings)
        t.set_triangle_uvs(uvs)
    t.clear_canvas()
    t.reset_denoise_history()
    if demod:
        t.set_denoise_demodulation(True)
    if illum:
        t.set_denoise_history_illumination(True)
    return t


def next_frame(t, cam, time, scn=None):
    """the front-end while moving: clear, update_scene, a new camera, one dispatch"""
    t.clear_canvas()
    t.update_scene(*(t.scene if scn is None else scn))
    t.options["camera_to_world"] = cam
    t.options["time"] = time
    return t.render(1).copy()


def same_history(a, b):
    assert a["valid"] == b["valid"]
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(a[k], b[k]), k


# ---- 1. the switch's rules -------------------------------------------------------------------------------------------------
def test_state_rules(T, sky):
    lib = T.load_library()
    w, h = 48, 32
    t = make(T, sky, "spheres", w, h, denoise=dict(iterations=0))
    assert lib.srt_set_denoise_history_illumination(t._h, 1) == SRT_ERR_STATE  # temporal reprojection is off
    assert lib.srt_set_denoise_history_illumination(t._h, 0) == 0
    with pytest.raises(T.SrtError):
        t.set_denoise_history_illumination(True)
    t.set_denoise_temporal()
    t.render(1)
    assert not t.last_setup_history_illumination()
    t.set_denoise_history_illumination(True)
    assert not t.last_setup_history_illumination()  # it takes effect at the next set-up
    t.resolve_denoised(1)  # K = 0 still runs the set-up, and its variant
    assert t.last_setup_history_illumination()
    t.clear_canvas()
    before = t.read_denoise_history()
    assert before["valid"]
    t.set_denoise_history_illumination(False)
    t.set_denoise_history_illumination(True)
    same_history(before, t.read_denoise_history())  # toggling clears nothing
    t.set_denoise_history_illumination(False)
    t.render(1)
    assert not t.last_setup_history_illumination()
    t.set_denoise_history_illumination(True)
    t.clear_canvas()  # the switch changed after the filter: the clear runs its own set-up, the variant the filter would run now
    assert t.last_setup_history_illumination()
    t.set_denoise_temporal(history_limit=16)  # another setting of the temporal stage: the switch stays
    t.render(1)
    assert t.last_setup_history_illumination()
    t.set_denoise_temporal(False)  # turning temporal off turns it off
    t.set_denoise_temporal()
    t.render(1)
    assert not t.last_setup_history_illumination()
    t.set_denoise_history_illumination(True)
    t.set_denoise(False)  # and so does turning the denoiser off
    t.set_denoise(iterations=0)
    t.set_denoise_temporal()
    t.render(1)
    assert not t.last_setup_history_illumination()
    t.close()
    p = T.Tracer(w, h)
    p.set_partition(0, 2)
    assert lib.srt_set_denoise_history_illumination(p._h, 1) == SRT_ERR_STATE  # never on a partitioned handle
    p.close()
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=8)
    assert lib.srt_group_set_denoise_history_illumination(g._g, 1) == SRT_ERR_STATE  # no denoiser yet
    assert lib.srt_group_set_denoise_history_illumination(g._g, 0) == 0
    assert not g.last_setup_history_illumination()
    g.close()
    g = handle(T, sky, "noise", w, h, group=2, illum=False)
    g.set_denoise_temporal(False)
    assert lib.srt_group_set_denoise_history_illumination(g._g, 1) == SRT_ERR_STATE  # the group's temporal reprojection is off
    g.set_denoise_temporal()
    g.set_denoise_history_illumination(True)
    g.render(1)
    assert g.last_setup_history_illumination()
    g.set_denoise_temporal(False)
    g.set_denoise_temporal()
    g.render(2)
    assert not g.last_setup_history_illumination()
    g.close()


def test_the_history_does_not_depend_on_whether_a_filter_ran(T, sky):
    """trace alone, then clear: the clear's own set-up is the variant the filter launches"""
    w, h = 64, 48
    a, b = (handle(T, sky, "noise", w, h) for _ in range(2))
    for k in range(3):
        for t in (a, b):
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(k, "move")
            t.options["time"] = 40 + k
        a.render(1)
        b.trace()
        for t in (a, b):
            t.clear_canvas()
            assert t.last_setup_history_illumination()
        same_history(a.read_denoise_history(), b.read_denoise_history())
    a.close()
    b.close()


# ---- 2. a still camera, 3. a scene of one colour: the switch-off bits --------------------------------------------------------
def on_equals_off(T, sky, kind, w, h, kind_of_path, frames=3):
    on, off = handle(T, sky, kind, w, h), handle(T, sky, kind, w, h, illum=False)
    for k in range(frames):
        outs = [next_frame(t, cam_at(k, kind_of_path), 700 + k) for t in (on, off)]
        assert on.last_setup_history_illumination() and not off.last_setup_history_illumination()
        assert np.array_equal(outs[0], outs[1]), k  # the ARGB bytes
        assert bits_equal(on.read_denoised(), off.read_denoised()), k  # the filter's input (K = 0: the set-up's output)
    for t in (on, off):
        t.clear_canvas()
    ha, hb = on.read_denoise_history(), off.read_denoise_history()
    same_history(ha, hb)
    assert ha["valid"] and (ha["count"] > 2).mean() > 0.3  # the history took part
    on.close()
    off.close()


def test_still_camera_is_bit_equal_to_the_switch_off(T, sky):
    on_equals_off(T, sky, "noise", 64, 48, None)


def test_one_colour_scene_is_bit_equal_to_the_switch_off(T, sky):
    on_equals_off(T, sky, "one-colour", 64, 48, "move")


# ---- 4. a moved camera against the restatement -------------------------------------------------------------------------------
POSES = ["dolly", "zoom_out", "roll", "big_yaw"]  # of temporal_cases: they carry the pose offset that avoids whole-pixel coordinates
MOVED_FRAMES = ([(kind, w, h) for kind in ("noise", "spheres", "mesh") for w, h in TC.SIZES] + [("noise", 1, 33), ("noise", 33, 1)])


@pytest.fixture(scope="module")
def pool(T, sky):
    made = {}

    def get(kind, w, h):
        if (kind, w, h) not in made:
            made[(kind, w, h)] = handle(T, sky, kind, w, h, tp=dict(TP, history_limit=64))
        return made[(kind, w, h)]

    yield get
    for t in made.values():
        t.close()


def aim(t, cam):
    m, fov, aspect = cam
    t.options["camera_to_world"] = m
    t.options["fov_scale"] = fov
    t.options["aspect_ratio"] = np.float32(t.width) / np.float32(t.height) if aspect is None else aspect


def check_setup(t, want, argb, label, exact_bits=True, got=None):
    """the frame just rendered (K = 0; got: its read_denoised() when another filter ran since) against want = history_illumination_ref.temporal_setup(), then the clear and the history
    it commits: bit for bit off the flagged pixels (exact_bits False: rtol 1e-4 there too), rtol 1e-4 on them, fewer than 0.1 %
    of the frame beyond that. -> the committed history"""
    w, h = t.width, t.height
    got = t.read_denoised() if got is None else got
    t.clear_canvas()
    assert t.last_setup_history_illumination()
    got_h = t.read_denoise_history()
    assert got_h["valid"]
    exact, close, worst = TC.compare_setup(want, got, argb.reshape(h, w, 4), got_h)
    border = want["rep"]["borderline"]
    print(f"{label} {w}x{h}: {int(border.sum())} pixels flagged, {int((~exact).sum())} differ in a bit ({int((~exact & ~border).sum())} unflagged, "
          f"at most {worst:.1f} ulp), {int((~close).sum())} beyond rtol 1e-4; {int((want['rep']['scaled'] > 0).sum())} pixels with a rescaled tap")
    bad = ~(exact if exact_bits else close) & ~border
    assert not bad.any(), (label, np.argwhere(bad)[:5])
    assert not (~close & ~border).any()
    assert int((~close & border).sum()) < 1e-3 * w * h, label
    return got_h


@pytest.mark.parametrize("kind,w,h", MOVED_FRAMES)
@pytest.mark.parametrize("name", POSES)
def test_moved_camera_matches_numpy(pool, name, kind, w, h):
    """a 2-spp frame at the history camera, clear, the current camera, a 2-spp frame: colour, variance, bytes and the committed
    history against the restatement fed the device's own canvas, inputs and history. The same frame's set-up with the switch
    off (the parent's kernel, run between the two) differs on more than a tenth of the pixels with taps. The cap on the
    restatement's own flagged share (under 0.1 % of a 128x72 frame for these poses and scenes) is asserted on the CPU, on the
    oracle's frames (tests/test_history_illumination_reference.py); the device's guide, from two jittered feature rays, flags up
    to 12 pixels of 9216 (dolly over the sphere scene), none of which differs."""
    tp = dict(TP, history_limit=64)
    t = pool(kind, w, h)
    hist_cam, cur_cam = TC.CASES[name]
    t.clear_canvas()
    t.reset_denoise_history()
    t.update_scene(*t.scene)
    aim(t, hist_cam)
    t.options["time"] = 2000
    t.render(1)
    t.clear_canvas()
    hist = t.read_denoise_history()
    assert hist["valid"]
    t.update_scene(*t.scene)
    aim(t, cur_cam)
    t.options["time"] = 2001
    argb = t.render(1).copy()
    assert t.last_setup_history_illumination() and t.last_trace_textured()
    inp = t.read_denoise_inputs()
    want = HI.temporal_setup(t.read_canvas(), inp, FS * inp["T"], hist, t.options, **tp)
    on = t.read_denoised()
    t.set_denoise_history_illumination(False)
    t.resolve_denoised(1)
    off = t.read_denoised()
    assert not t.last_setup_history_illumination()
    t.set_denoise_history_illumination(True)  # (the clear in check_setup runs the illumination set-up again for the commit)
    check_setup(t, want, argb, f"{name} {kind}", got=on)
    if (w, h) in TC.SIZES:
        has = want["rep"]["taps"] > 0
        differ = has & ~TC.same_bits(on[..., :3], off[..., :3])
        print(f"{name} {kind} {w}x{h}: {int(has.sum())} pixels with taps, {int(differ.sum())} differ from the switch-off set-up")
        assert has.sum() > 0.1 * w * h and differ.sum() > 0.1 * has.sum()


# ---- 5. object motion and per-triangle motion ----------------------------------------------------------------------------------
def test_moved_textured_sphere_matches_numpy(T, sky):
    w, h = 64, 48
    tp = dict(TP, history_limit=64)
    t = handle(T, sky, "spheres", w, h, tp=tp, motion=True)
    shapes, tris, mats = t.scene
    big = int(np.flatnonzero(shapes["material"] == 3)[0])  # the striped sphere
    steps = [(big, "translate", (0.031, 0.012, 0.02))]
    t.options["camera_to_world"] = cam_at(0, "move")
    t.render(1)
    t.clear_canvas()
    hist = t.read_denoise_history()
    hist["ids"] = t.read_denoise_shape_ids()[1]
    t.update_scene(M.move_shapes(shapes, tris, steps, 1), tris, mats)
    table = t.read_denoise_motion()
    assert t.read_denoise_history()["valid"] and table["any_moved"]
    t.options["camera_to_world"] = cam_at(1, "move")
    t.options["time"] = 2001
    argb = t.render(1).copy()
    ids = t.read_denoise_shape_ids()[0]
    inp = t.read_denoise_inputs()
    want = HI.temporal_setup(t.read_canvas(), inp, FS * inp["T"], hist, t.options, ids=ids, table=table, **tp)
    check_setup(t, want, argb, "a moved textured sphere")
    kept = (ids == big) & (want["h"] > 0)
    assert kept.any() and (want["rep"]["state"][ids == big] == M.MOVED).all() and (want["rep"]["scaled"][kept] > 0).any()
    t.close()


def test_waving_textured_mesh_matches_numpy(T, sky):
    """the deform kernel's variant; §17's comparison (rtol 1e-4 off the flagged pixels: the per-triangle map is not held to bits)"""
    w, h = 64, 48
    tp = dict(TP, history_limit=64)
    t = handle(T, sky, "mesh", w, h, tp=tp, vertex=True)
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
    assert table["state"].tolist() == want_table["state"].tolist()
    table["first_row"] = want_table["first_row"]
    t.options["time"] = 2001
    argb = t.render(1).copy()
    ids, tri_ids = t.read_denoise_shape_ids()[0], t.read_denoise_triangle_ids()[0]
    rows = t.read_denoise_vertex_tables()[0]
    inp = t.read_denoise_inputs()
    want = HI.temporal_setup(t.read_canvas(), inp, FS * inp["T"], hist, t.options, ids=ids, table=table, tri_ids=tri_ids, rows=rows, h_rows=h_rows, **tp)
    assert want["rep"]["borderline"].mean() <= 0.01
    check_setup(t, want, argb, "a waving textured mesh", exact_bits=False)
    on = want["rep"]["state"] == V.DEFORMED
    assert (on & (want["h"] > 0)).any() and (want["rep"]["scaled"][on] > 0).any()
    t.close()


# ---- 6. demodulation and the spatial variance estimate on top ---------------------------------------------------------------------
def test_filter_with_demodulation_and_spatial_variance_matches_numpy(T, sky):
    w, h, K, ms = 64, 48, 5, 8
    t = handle(T, sky, "noise", w, h, K=K, demod=True, cam=cam_at(0, "move"))
    t.set_denoise_spatial_variance(ms)
    t.render(1)
    t.clear_canvas()
    hist = t.read_denoise_history()
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam_at(3, "move")
    t.options["time"] = 2001
    argb = t.render(1).copy().reshape(h, w, 4)
    assert t.last_setup_history_illumination() and t.last_filter_demodulated() and t.last_filter_spatial_variance()
    got = t.read_denoised()
    inp = t.read_denoise_inputs()
    want = HI.temporal_setup(t.read_canvas(), inp, FS * inp["T"], hist, t.options, **TP)
    cur = want["cur"]
    st = dict(c=want["c"], V=want["V"], N=cur["N"], Z=cur["Z"], A=cur["A"], cov=cur["cov"], src=SV.sources_staged(want["commit"]),
              commit=want["commit"], borderline=want["rep"]["borderline"])
    t.clear_canvas()
    adopt_staged(st, t.read_denoise_history())  # (a flagged pixel the library decided the other way: its staged values)
    steps, _ = SV.filter_steps(st["c"], st["V"], st["N"], st["Z"], st["A"], st["cov"], *st["src"], ms, iterations=K, demod=True)
    check_filter(got, argb, *steps[K], "demodulation + spatial variance over the illumination set-up")
    assert (want["rep"]["scaled"] > 0).sum() > 0.3 * w * h
    t.close()


# ---- 7. a device group ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_handle(T, sky, n):
    w, h = 48, 40
    single, group = handle(T, sky, "noise", w, h, K=2), handle(T, sky, "noise", w, h, K=2, group=n)
    for k in range(3):
        outs = []
        for t in (single, group):
            t.clear_canvas()
            t.options["camera_to_world"] = cam_at(k, "yaw")
            t.options["time"] = 500 + k
            outs.append(t.render(1).copy())
            assert t.last_setup_history_illumination()
        assert np.array_equal(outs[0], outs[1]), k
        assert bits_equal(single.read_denoised(), group.read_denoised()), k
    for t in (single, group):
        t.clear_canvas()
    same_history(single.read_denoise_history(), group.read_denoise_history())
    for t in (single, group):
        t.set_denoise_history_illumination(False)
    assert np.array_equal(single.render(1), group.render(1)) and not group.last_setup_history_illumination()
    single.close()
    group.close()


# ---- 8., 9. quality ----------------------------------------------------------------------------------------------------------------
# Measured on an MI355X (160x90, eight 2-spp frames along the moving camera of tests/test_gpu_denoise_temporal.py, tonemapped MSE of
# the last frame against 4096 spp at its camera; profiles/r19_history_illumination_quality.json):
TEXTURED_QUALITY = dict(off=3.8800e-03, on=3.8720e-03, ratio=0.9979)  # the threshold is halfway between ratio and 1 (0.99895)
# 0.9979 is not clearly below 1: on this scene (a texel per pixel, 2 spp) the switch changes the error by 0.2 %, so no quality
# claim is made for it. The spatial filter alone stands at 4.2981e-03: the history as a whole removes a tenth here.


def moving_camera(T, sky, kind, K, demod, frames=8, w=160, h=90):
    """-> (reference tone image, switch-off result, switch-on result, the pixels no history reached)"""
    last = cam_at(frames - 1, "move")
    g = handle(T, sky, kind, w, h, illum=False, cam=last, time=4242)
    g.options["num_samples"] = 4096
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    off, on = handle(T, sky, kind, w, h, K=K, demod=demod, illum=False), handle(T, sky, kind, w, h, K=K, demod=demod)
    for k in range(frames):
        for t in (off, on):
            next_frame(t, cam_at(k, "move"), 900 + k)
    assert on.last_setup_history_illumination() and not off.last_setup_history_illumination()
    a, b = off.read_denoised()[..., :3], on.read_denoised()[..., :3]
    on.clear_canvas()
    hist = on.read_denoise_history()
    dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)
    off.close()
    on.close()
    return ref, a, b, dis


def test_textured_quality_moving_camera(T, sky):
    """scenes.textured_noise_scene, demodulation on, K = 5: the switch on against the switch off (the parent's behaviour)"""
    ref, off, on, _ = moving_camera(T, sky, "noise", 5, True)
    mse_off, mse_on = float(np.mean((tone(off) - ref) ** 2)), float(np.mean((tone(on) - ref) ** 2))
    print(f"noise texture, moving camera: switch off MSE {mse_off:.4e}, on {mse_on:.4e}, ratio {mse_on / mse_off:.4f}")
    assert mse_on < mse_off
    assert TEXTURED_QUALITY is not None, "the ratio has not been measured yet"
    assert mse_on / mse_off <= (TEXTURED_QUALITY["ratio"] + 1.0) / 2.0


@pytest.mark.parametrize("kind", ["spheres", "meshes"])
def test_untextured_quality_keeps_the_temporal_thresholds(T, sky, kind):
    """tests/test_gpu_denoise_temporal.py test_quality_moving_camera's scenes and thresholds with the switch on (its set-up: the
    default denoiser, one feature sample); the on / off ratio is printed, no claim"""
    w, h, frames = 160, 90, 8
    accel = 1 if kind == "meshes" else 0
    g = make(T, sky, kind, w, h, spp=4096, accel=accel, time=4242)
    g.options["camera_to_world"] = cam_at(frames - 1, "move")
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    sp = make(T, sky, kind, w, h, accel=accel, denoise={})
    off = make(T, sky, kind, w, h, accel=accel, denoise={}, temporal={})
    on = make(T, sky, kind, w, h, accel=accel, denoise={}, temporal={})
    on.set_denoise_history_illumination(True)
    for k in range(frames):
        for t in (sp, off, on):
            next_frame(t, cam_at(k, "move"), 900 + k)
    assert on.last_setup_history_illumination()
    a, b, c = (t.read_denoised()[..., :3] for t in (sp, off, on))
    on.clear_canvas()
    hist = on.read_denoise_history()
    dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)
    mse = lambda x, m=slice(None): float(np.mean((tone(x)[m] - ref[m]) ** 2))
    print(f"{kind}: spatial MSE {mse(a):.3e}, temporal {mse(b):.3e}, with the switch {mse(c):.3e} (on / off {mse(c) / mse(b):.4f}); "
          f"pixels without history: {mse(c, dis) / mse(a, dis):.3f} of the spatial filter's")
    assert mse(c) <= 0.7 * mse(a)
    assert dis.any() and mse(c, dis) <= 1.25 * mse(a, dis)
    for t in (sp, off, on):
        t.close()


# ---- srt_headless ------------------------------------------------------------------------------------------------------------------
def test_headless_history_illumination_writes_another_frame(tmp_path):
    """srt_headless --denoise 5 --temporal --move --history-illumination on a textured scene: a frame comes out, and it is not the
    frame without the switch"""
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    img = np.random.default_rng(9).integers(0, 256, (16, 16, 3)).astype(np.uint8)
    ppm = tmp_path / "tex.ppm"
    ppm.write_bytes(b"P6\n16 16\n255\n" + img.tobytes())
    frames = []
    for extra in ([], ["--history-illumination"]):
        out = tmp_path / f"f{len(extra)}.ppm"
        subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "48", "--spp", "2", "--frames", "3", "--denoise", "5", "--temporal",
                        "--move", "0.05", "--texture", str(ppm), "--texture-material", "0", "--texture-scale", "4", "--texture-nearest",
                        "--out", str(out)] + extra, check=True, timeout=120)
        frames.append(out.read_bytes())
    assert frames[1].startswith(b"P6") and len(frames[0]) == len(frames[1]) > 64 * 48 * 3
    assert frames[0] != frames[1]
