"""The ID pass and the selection overlay on the device (include/srt_abi.h "selection overlay and the ID pass"; csrc/selection.hip):
the ID planes against srt_pick of every pixel centre bit for bit under every acceleration mode, what the pass leaves
untouched, and the overlaid bytes and the alpha plane against the numpy restatement (tests/selection_ref.py) applied to the
bytes of the same frame without a selection and the ID plane read from the device -- every comparison is of integers.

The outline cases' cameras were chosen on the CPU (pixel-centre rays of the sphere scene, in numpy) so that the selected mask has
the share its case is about; every case asserts that share on the ID plane the device made, so no case passes on an empty mask.
Frames are 70x37: neither side is a multiple of 64, of the outline kernel's 32x8 tile or of 8."""
import subprocess

import numpy as np
import pytest

import gpu_harness as G
import selection_ref as SR
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import frame_rd, scene
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
W, H, SPP, TIME = 70, 37, 1, 777
DEVICE, MEDIAN = 1, 1
OUTLINE, FILL = (200, 255, 160, 0), (96, 40, 90, 250)  # A, R, G, B; the outline is not opaque, so a wrong blend shows at every alpha
CAM_A = S.default_camera()  # with fov 0.25: sphere 4 in the middle, sphere 3 cut by the left and bottom borders, 5 by the right one
CAM_C = R.camera_matrix((3.0, 0.5, 5.0), 0.45, 0.0)  # with fov 0.35: sphere 5 in front of sphere 4, touching it in the image
CAM_CORNER = R.camera_matrix((0.14, 0.5, 5.0), 0.0, 0.0)  # with fov 0.25: sphere 4's rim runs through the tile corner (32, 8)
CAM_FLOOR = R.camera_matrix((20.0, 3.0, 20.0), 0.0, -1.5)  # looks down on the floor plane, far from everything else

# name -> camera, fov, selected shapes, frame, (lowest, highest) share of the selected mask
CASES = {
    "sphere": (CAM_A, 0.25, [4, 1000], (W, H), (0.02, 0.60)),  # 1000: beyond the scene, kept and never matches
    "tile_corner": (CAM_CORNER, 0.25, [4], (W, H), (0.02, 0.60)),
    "cut_by_border": (CAM_A, 0.25, [3], (W, H), (0.02, 0.60)),
    "off_screen": (CAM_A, 0.08, [6], (W, H), (0.0, 0.0)),
    "floor_fills_frame": (CAM_FLOOR, 0.3, [0], (W, H), (1.0, 1.0)),
    "two_touching": (CAM_C, 0.35, [4, 5], (W, H), (0.02, 0.60)),
    "partly_hidden": (CAM_C, 0.35, [4], (W, H), (0.02, 0.60)),
    "frame_1x1": (CAM_A, 0.25, [4], (1, 1), (1.0, 1.0)),  # the one pixel is sphere 4
    "frame_3x2": (CAM_A, 0.25, [4], (3, 2), (0.02, 0.60)),  # one pixel of six
}
MAIN = ("sphere", "tile_corner", "cut_by_border", "two_touching", "partly_hidden")


def rd_of(cam, fov, w=W, h=H, time=TIME):
    return frame_rd(cam, w, h, SPP, time, fov)


def make(T, sky, w=W, h=H, cam=CAM_A, fov=0.25, shapes=None, **kw):
    sh, tr, ma = scene("spheres")
    t = G.make(T, sky, (sh if shapes is None else shapes, tr, ma), w, h, spp=SPP, time=TIME, **kw)
    t.options = rd_of(cam, fov, w, h)
    return t


def frame(t, ticks=1):
    t.clear_canvas()
    return t.render(ticks).reshape(t.height, t.width, 4).copy()


def expect(off, ids, sel, width, outline=OUTLINE, fill=FILL, n_shapes=7):
    return SR.apply(off, ids["shape"], sel, n_shapes, width, outline, fill)


# ---- 1. the ID pass ---------------------------------------------------------------------------------------------------------------
def id_handle(T, name, accel):
    sh, tr, ma = scene(name)
    t = T.Tracer(W, H)
    t.set_acceleration(0 if accel == "scan" else 1)
    if accel == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    return t, sh


ID_CASES = [("spheres", "scan", CAM_A, 0.25), ("boxes", "scan", R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15), 1.0),
            ("boxes", "sah", R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15), 1.0),
            ("mesh_smooth", "scan", R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0), 0.5), ("mesh_smooth", "sah", R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0), 0.5),
            ("mesh_smooth", "median", R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0), 0.5)]


@pytest.mark.parametrize("name,accel,cam,fov", ID_CASES, ids=[f"{c[0]}-{c[1]}" for c in ID_CASES])
def test_id_planes_equal_pick_of_every_pixel_centre(name, accel, cam, fov, T):
    t, sh = id_handle(T, name, accel)
    rd = rd_of(cam, fov)
    xy = np.array([(px + 0.5, py + 0.5) for py in range(H) for px in range(W)], np.float32)
    picked = t.pick(xy, options=rd)
    t.render_ids(rd)
    ids = t.read_id_pass()
    assert ids["shape"].shape == (H, W) and len(picked) == 2590
    for plane in ("shape", "triangle", "material"):
        assert np.array_equal(ids[plane].reshape(-1), picked[plane]), (name, accel, plane)
    hit = picked["shape"] != R.HIT_NONE
    assert len(np.unique(picked["shape"][hit])) >= 3, "the frame shows several shapes"
    if name != "spheres":
        on_model = picked["triangle"] != R.HIT_NONE
        assert on_model.sum() >= 64 and (~on_model).sum() >= 64 and len(np.unique(picked["triangle"][on_model])) >= 4
        assert (sh["type"][picked["shape"][on_model]] == R.SHAPE_MODEL).all()
    t.close()


def test_id_pass_reports_a_shape_without_a_material_and_misses(T):
    sh, tr, ma = scene("spheres")
    sh = sh.copy()
    sh["material"][4] = -1
    keep = np.array([3, 4, 5, 6])  # no planes: the rays beside the spheres miss
    t = T.Tracer(W, H)
    t.scene_data = R.scene_data(len(keep))
    t.update_scene(sh[keep], tr, ma)
    rd = rd_of(CAM_A, 0.25)
    t.render_ids(rd)
    ids = t.read_id_pass()
    on4 = ids["shape"] == 1
    assert on4.sum() >= 100 and (ids["material"][on4] == -1).all() and (ids["triangle"][on4] == R.HIT_NONE).all()
    miss = ids["shape"] == R.HIT_NONE
    assert miss.sum() >= 100 and (ids["triangle"][miss] == R.HIT_NONE).all() and (ids["material"][miss] == -1).all()
    picked = t.pick([(px + 0.5, py + 0.5) for py in range(H) for px in range(W)], options=rd)
    assert np.array_equal(ids["shape"].reshape(-1), picked["shape"]) and np.array_equal(ids["material"].reshape(-1), picked["material"])
    t.close()


def test_id_pass_leaves_canvas_counters_and_trace_answers_alone(T, sky):
    t = make(T, sky)
    t.set_kernel_timers(True)
    t.render(1)
    before = (t.counters(), t.read_canvas().copy(), t.last_trace_launches(), t.last_trace_class(), t.last_trace_textured(), t.last_trace_plane_form(),
              t.last_trace_kernel_ms(), t.last_kernel_ms(), t.read_argb().copy())
    t.render_ids(rd_of(CAM_C, 0.35))
    t.render_ids()
    t.read_id_pass()
    after = (t.counters(), t.read_canvas(), t.last_trace_launches(), t.last_trace_class(), t.last_trace_textured(), t.last_trace_plane_form(),
             t.last_trace_kernel_ms(), t.last_kernel_ms(), t.read_argb())
    assert before[0] == after[0] and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert before[2:8] == after[2:8] and np.array_equal(before[8], after[8])
    assert t.last_resolve_selected() == (False, False)
    t.close()


def test_id_pass_arguments(T):
    t = T.Tracer(W, H)
    with pytest.raises(T.SrtError):
        t.read_id_pass()  # no pass yet
    lib = t.lib
    assert lib.srt_render_ids(t._h, None) != 0 and lib.srt_render_ids(None, None) != 0
    bad = rd_of(CAM_A, 0.25)
    bad["width"] = 0
    with pytest.raises(T.SrtError):
        t.render_ids(bad)
    t.scene_data = R.scene_data(7)
    t.update_scene(*scene("spheres"))
    t.render_ids(rd_of(CAM_A, 0.25, 5, 3))  # any frame size
    assert t.read_id_pass()["shape"].shape == (3, 5)
    small = np.zeros(14, np.uint32)
    assert lib.srt_read_id_pass(t._h, T._ptr(small), None, None, 14, None, None) != 0  # 15 pixels do not fit
    t.close()


# ---- 2. outline and composite --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def off_frames(T, sky):
    """per case: the bytes without a selection and the ID planes of the case's camera (rendered once, shared, never changed)"""
    out = {}
    for name, (cam, fov, sel, (w, h), share) in CASES.items():
        t = make(T, sky, w, h, cam, fov)
        off = frame(t)
        assert t.last_resolve_selected() == (False, False)
        t.render_ids()
        out[name] = (off, t.read_id_pass())
        t.close()
    return out


def check_case(T, sky, off_frames, name, width, fill_alpha):
    cam, fov, sel, (w, h), (lo, hi) = CASES[name]
    off, ids = off_frames[name]
    fill = (fill_alpha,) + FILL[1:]
    t = make(T, sky, w, h, cam, fov)
    t.set_selection(sel, width=width, outline=OUTLINE, fill=fill)
    on = frame(t)
    assert t.last_resolve_selected() == (True, True)
    got_ids, alpha = t.read_id_pass(), t.read_selection_alpha()
    for plane in ids:
        assert np.array_equal(got_ids[plane], ids[plane]), (name, plane)
    want, want_alpha, m = expect(off, ids, sel, width, fill=fill)
    share = m.mean()
    assert lo <= share <= hi, (name, share)
    assert np.array_equal(alpha, want_alpha), name
    assert np.array_equal(on, want), name
    assert np.array_equal(on[..., 0], off[..., 0])  # the picture's alpha byte stays
    assert np.array_equal(on[alpha == 0], off[alpha == 0])
    t.close()
    return off, on, alpha, m


@pytest.mark.parametrize("fill_alpha", [0, 96])
@pytest.mark.parametrize("width", [1.0, 3.0, 8.0])
@pytest.mark.parametrize("name", MAIN)
def test_overlay_equals_the_restatement(name, width, fill_alpha, T, sky, off_frames):
    off, on, alpha, m = check_case(T, sky, off_frames, name, width, fill_alpha)
    ring = ~m & (alpha != 0)
    assert ring.sum() >= 8 and ((alpha[ring] > 0) & (alpha[ring] < OUTLINE[0])).any(), "a partly covered outline pixel"
    assert (alpha[m] == fill_alpha).all() and not np.array_equal(on, off)
    if name == "tile_corner":  # the four pixels around the first interior corner of the 32x8 tiling hold both sides of the rim
        around = m[7:9, 31:33]
        assert around.any() and not around.all(), around
    if name == "cut_by_border":
        assert m[:, 0].any() and m[-1, :].any(), "the shape reaches the frame's left and bottom edge"
    if name == "two_touching":
        ids = off_frames[name][1]["shape"]
        beside = (ids[:, :-1] == 4) & (ids[:, 1:] == 5)
        assert beside.sum() >= 4, "the two spheres are neighbours in the image"
        assert (alpha[:, :-1][beside] == fill_alpha).all() and (alpha[:, 1:][beside] == fill_alpha).all()  # no outline between them
    if name == "partly_hidden":
        ids = off_frames[name][1]["shape"]
        beside = (ids[:, :-1] == 4) & (ids[:, 1:] == 5)  # sphere 5 stands in front: its pixels beside the visible part are outline
        assert beside.sum() >= 4 and (alpha[:, 1:][beside] == SR.table(width, OUTLINE[0])[0][1]).all()


def test_selected_shape_off_screen_writes_nothing(T, sky, off_frames):
    off, on, alpha, m = check_case(T, sky, off_frames, "off_screen", 3.0, 96)
    assert not m.any() and not alpha.any() and np.array_equal(on, off)


def test_floor_plane_fills_every_pixel(T, sky, off_frames):
    off, on, alpha, m = check_case(T, sky, off_frames, "floor_fills_frame", 3.0, 96)
    assert m.all() and (alpha == 96).all() and (on[..., 1:] != off[..., 1:]).any()
    check_case(T, sky, off_frames, "floor_fills_frame", 3.0, 0)  # no fill: nothing is written


@pytest.mark.parametrize("name", ["frame_1x1", "frame_3x2"])
def test_halo_larger_than_the_frame(name, T, sky, off_frames):
    """width 8 reaches across the whole frame: every unselected pixel is within 8.5 - 1 pixels of a selected one, so its alpha is
    the outline's full one (no partly covered pixel can exist at these sizes)"""
    off, on, alpha, m = check_case(T, sky, off_frames, name, 8.0, 96)
    assert m.any() and (alpha[m] == 96).all() and (alpha[~m] == OUTLINE[0]).all()


# ---- 3. when the ID pass runs ------------------------------------------------------------------------------------------------------
def test_id_pass_is_cached_until_scene_or_camera_change(T, sky):
    sh, tr, ma = scene("spheres")
    t = make(T, sky)
    t.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    frame(t)
    assert t.last_resolve_selected() == (True, True)
    frame(t)
    assert t.last_resolve_selected() == (True, False)
    t.options["time"] = np.uint32(999)  # not part of the key
    frame(t)
    assert t.last_resolve_selected() == (True, False)
    moved = sh.copy()
    moved["sphere_position"][4][:3] = (-0.2, 0.6, -3.0)
    t.update_scene(moved, tr, ma)
    on = frame(t)
    assert t.last_resolve_selected() == (True, True)
    ids, alpha = t.read_id_pass(), t.read_selection_alpha()
    t.set_selection()
    off = frame(t)
    assert t.last_resolve_selected() == (False, False)
    want, want_alpha, m = expect(off, ids, [4], 3.0)
    assert 0.02 <= m.mean() <= 0.60 and np.array_equal(on, want) and np.array_equal(alpha, want_alpha)
    old = make(T, sky)
    old.render_ids()
    assert not np.array_equal(old.read_id_pass()["shape"], ids["shape"]), "the planes are the moved scene's"
    old.close()
    t.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    frame(t)
    assert t.last_resolve_selected() == (True, False)  # the planes survived the switch
    t.options = rd_of(CAM_C, 0.35)
    frame(t)
    assert t.last_resolve_selected() == (True, True)
    t.options = rd_of(CAM_C, 0.36)
    frame(t)
    assert t.last_resolve_selected() == (True, True)
    t.close()


def test_no_overlay_before_a_dispatch(T, sky):
    t = make(T, sky)
    t.set_selection([4])
    t.resolve(1)
    assert t.last_resolve_selected() == (False, False)
    t.trace()
    t.resolve(1)
    assert t.last_resolve_selected() == (True, True)
    t.close()


# ---- 4. the other sites --------------------------------------------------------------------------------------------------------
def test_every_site_gives_the_same_bytes(T, sky, off_frames):
    off, ids = off_frames["sphere"]
    want = expect(off, ids, [4], 3.0)[0].reshape(-1)
    t = make(T, sky)
    t.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    out = {}
    t.clear_canvas()
    t.trace()
    t.resolve(1)
    out["trace + resolve"] = t.read_argb().copy()
    t.clear_canvas()
    buf = np.zeros(W * H * 4, np.uint8)
    t.render_async(1, buf)
    t.synchronize()
    out["render_async"] = buf
    canvas = t.read_canvas()
    ext = t.device_buffers()
    t.resolve_external(ext[0], W * H, 1, ext[2])  # keeps its bytes unchanged
    out_ext = t.read_argb().copy()
    assert np.array_equal(out_ext.reshape(H, W, 4), off) and np.array_equal(canvas.view(np.uint32), t.read_canvas().view(np.uint32))
    for site, b in out.items():
        assert np.array_equal(np.asarray(b).reshape(-1), want), site
    t.close()


def test_pipelined_frames_equal_blocking_frames(T, sky):
    runs = []
    for pipelined in (False, True):
        t = make(T, sky)
        t.set_selection([4, 5], width=2.0, outline=OUTLINE, fill=FILL)
        frames, bufs = [], [np.zeros(W * H * 4, np.uint8) for _ in range(9)]
        for k in range(8):
            t.options = rd_of(CAM_C if k >= 4 else CAM_A, 0.35 if k >= 4 else 0.25, time=TIME + 31 * k)  # the camera changes once on the way
            if pipelined:
                if t.render_pipelined(k + 1, bufs[k]) >= 0:
                    frames.append(bufs[k].copy())
            else:
                frames.append(t.render(k + 1).copy())
        if pipelined:
            t.synchronize()
            assert t.pipeline_flush(bufs[8]) == 7
            frames.append(bufs[8].copy())
        assert t.last_resolve_selected() == (True, False)
        runs.append(frames)
        t.close()
    blocking, piped = runs
    assert len(blocking) == 8 and len(piped) == 8  # frames 0..6 delivered on the way, 7 by the flush
    for k in range(8):
        assert np.array_equal(piped[k], blocking[k]), k


def test_behind_denoiser_exposure_and_bloom(T, sky):
    frames = {}
    for on in (False, True):
        t = make(T, sky, denoise=dict(iterations=2))
        t.set_exposure(mode="manual", ev=1.0)
        t.set_bloom(threshold=0.2, knee=0.1, intensity=0.5)
        if on:
            t.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
        frames[on] = frame(t)
        assert t.last_resolve_bloomed() and t.last_resolve_exposed() and t.last_resolve_selected()[0] == on
        if on:
            ids, alpha = t.read_id_pass(), t.read_selection_alpha()
            t.resolve_denoised(1)
            assert np.array_equal(t.read_argb().reshape(H, W, 4), frames[True])
        t.close()
    want, want_alpha, m = expect(frames[False], ids, [4], 3.0)
    assert 0.02 <= m.mean() <= 0.60 and np.array_equal(alpha, want_alpha)
    assert np.array_equal(frames[True], want)


@pytest.mark.parametrize("denoise", [False, True], ids=["gathered", "denoised"])
def test_group_gives_the_single_handles_bytes(denoise, T, sky):
    single = make(T, sky, **(dict(denoise=dict(iterations=1)) if denoise else {}))
    single.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    want = frame(single)
    ids = single.read_id_pass()
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
    g.set_skybox(sky)
    g.options, g.scene_data = single.options.copy(), single.scene_data.copy()
    g.update_scene(*single.scene)
    single.close()
    g.clear_canvas()
    if denoise:
        g.set_denoise(iterations=1)
    assert g.last_resolve_selected() == (False, False)
    g.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    got = g.render(1).reshape(H, W, 4)
    assert g.last_resolve_selected() == (True, True)
    assert np.array_equal(g.read_id_pass()["shape"], ids["shape"])
    assert np.array_equal(got, want)
    g.clear_canvas()
    g.render(1)
    assert g.last_resolve_selected() == (True, False)
    g.close()


def test_partitioned_member_is_not_overlaid(T, sky):
    t = make(T, sky)
    t.set_partition(0, 2, 8)
    t.set_selection([4])
    t.clear_canvas()
    t.render(1)
    assert t.last_resolve_selected() == (False, False)
    t.close()


def test_switch_off_equals_a_handle_that_never_had_one(T, sky, off_frames):
    off, _ = off_frames["sphere"]
    t = make(T, sky)
    t.set_selection([4], width=3.0, outline=OUTLINE, fill=FILL)
    assert not np.array_equal(frame(t), off)
    t.set_selection([])
    assert np.array_equal(frame(t), off) and t.last_resolve_selected() == (False, False)
    t.set_selection([4], enabled=0)
    assert np.array_equal(frame(t), off) and t.last_resolve_selected() == (False, False)
    with pytest.raises(T.SrtError):
        t.set_selection([4], width=0.5)
    with pytest.raises(T.SrtError):
        t.set_selection([4], reserved=[0, 1, 0, 0])
    t.close()


# ---- 5. the headless route -------------------------------------------------------------------------------------------------------
def test_headless_select_writes_the_python_paths_bytes(T, tmp_path):
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    prefix, ppm = str(tmp_path / "s"), tmp_path / "f.ppm"
    cmd = [exe, "--scene", "spheres", "--width", str(W), "--height", str(H), "--spp", "1", "--bounces", "2", "--frames", "1", "--select", "0:3",
           "--out", str(ppm), "--dump", prefix]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    assert "selection: 1 shape(s)\n" in out, out
    data = ppm.read_bytes()
    header = f"P6 {W} {H} 255\n".encode()
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)
    t = T.Tracer(W, H)
    t.set_skybox(np.fromfile(prefix + ".sky.bin", np.float32).reshape(1024, 2048, 4))
    t.options = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    t.scene_data = np.fromfile(prefix + ".sd.bin", R.SCENE_DATA)[0]
    t.update_scene(np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    t.clear_canvas()
    plain = t.render(1).reshape(H, W, 4).copy()
    t.set_selection([0], width=3.0)
    t.clear_canvas()
    got = t.render(1).reshape(H, W, 4)
    assert np.array_equal(got[..., 1:], rgb) and not np.array_equal(got, plain)
    share = (t.read_id_pass()["shape"] == 0).mean()
    assert 0.02 <= share <= 0.60, share
    t.close()
