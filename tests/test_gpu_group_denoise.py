"""GPU (MI355X): the denoiser on a device group (srt_group_set_denoise and friends; csrc/srt_group.hip).

The members accumulate the filter's inputs for their own rows, one collective brings canvas rows and inputs to the first
device, one unpermute launch puts them in image order and the single handle's filter runs there. Nothing of that has an
atomic and every input is seeded by the global pixel index, so the reference of every test is a single Tracer of the same
size given the same call sequence, and equality is bit for bit (bits_equal on floats, array_equal on bytes). The N > 1 path
runs on VIRTUAL devices (devices=[0] * n: N members on the one GPU, a device-to-device copy where ncclGather sits), the RCCL
leg with a group of one device.

Frames are 64x48, 64x40 and 61x29 (ragged in both directions). Against n members x rows_per_block these give whole rounds
of blocks (2 x 8 of 48), a ragged last round (3 x 5 of 40: 8 blocks), a one-row last block with single-digit blocks per
member (5 x 2 of 29), single-row blocks (8 x 1 of 29: the last round has 5 of 8 members) and members that own nothing
(8 x 8 of 48: 6 blocks)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import bits_equal
from gpu_harness import T, cam_at, guide_scene  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu

GRID = [(2, 8, 64, 48), (3, 5, 64, 40), (5, 2, 61, 29), (8, 1, 61, 29), (8, 8, 64, 48)]  # members, rows per block, width, height
SCENES = [("spheres", 0), ("mixed", 0), ("mesh_flat", 0), ("mesh_flat", 1)]  # name, acceleration (mesh: array scan and BVH)
FS_NS = [(1, 1), (1, 2), (1, 4), (3, 1), (3, 2), (3, 4)]  # feature_samples, num_samples (3 > 1, 2: num_samples < feature_samples)
INPUT_KEYS = ("normal_depth", "albedo_hits", "moments")
DISPATCHES = 3


def build(T, sky, n, rpb, w, h, scene, accel, ns, cam=None, time=777, virtual=True):
    """A tracer over the scene, cleared: n == 0 the single handle (the reference), else a group of n virtual devices
    (virtual=False: no device list, devices 0 .. n - 1 and their RCCL communicator)."""
    shapes, tris, mats, scam = guide_scene(scene)
    t = T.Tracer(w, h) if n == 0 else T.TracerGroup(w, h, n_devices=n, devices=[0] * n if virtual else None, rows_per_block=rpb)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, ns, 10, camera_to_world=scam if cam is None else cam, time=time)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.scene = (shapes, tris, mats)
    return t


def set_budget(T, t, n, nbytes):
    lib = T.load_library()
    if n == 0:
        t.set_radiance_budget(nbytes)
    else:
        for i in range(n):
            assert lib.srt_set_radiance_budget(t.member(i), nbytes) == 0


_RUNS = {}


def run(T, sky, n, rpb, w, h, scene, accel, fs, ns, K, budget=0):
    """DISPATCHES dispatches without a clear between them; after each: the render's bytes, the filter's inputs and counts,
    the filtered image and the canvas. K None: the denoiser stays off (bytes and canvas only). Computed once per
    configuration and shared (the single handle's: by every group shape of that frame size)."""
    key = (n, rpb if n else 0, w, h, scene, accel, fs, ns, K, budget)
    if key in _RUNS:
        return _RUNS[key]
    t = build(T, sky, n, rpb, w, h, scene, accel, ns)
    if K is not None:
        t.set_denoise(iterations=K, feature_samples=fs)
    if budget:
        set_budget(T, t, n, budget)
    out = []
    for d in range(DISPATCHES):
        t.options["time"] = np.uint32(777 + 31 * d)
        rec = {"bytes": t.render(d + 1).copy(), "canvas": t.read_canvas()}
        if K is not None:
            rec["inputs"] = t.read_denoise_inputs()
            rec["denoised"] = t.read_denoised()
        out.append(rec)
    t.close()
    _RUNS[key] = out
    return out


def same_inputs(got, want, what):
    for d, (g, s) in enumerate(zip(got, want)):
        for k in INPUT_KEYS:
            assert bits_equal(g["inputs"][k], s["inputs"][k]), (what, d + 1, k)
        assert (g["inputs"]["T"], g["inputs"]["P"]) == (s["inputs"]["T"], s["inputs"]["P"]) and g["inputs"]["T"] == d + 1, (what, d + 1)


# ---- 1. the filter's inputs ----------------------------------------------------------------------------------------------
# every scene on every group shape; the (feature_samples, num_samples) pairs go round with the case number
INPUT_CASES = [(scene, accel, *GRID[g], *FS_NS[(g + 2 * s) % len(FS_NS)]) for s, (scene, accel) in enumerate(SCENES) for g in range(len(GRID))]
# ... and every pair on the sphere scene's ragged-round shape
INPUT_CASES += [("spheres", 0, *GRID[1], fs, ns) for fs, ns in FS_NS if ("spheres", 0, *GRID[1], fs, ns) not in INPUT_CASES]


@pytest.mark.parametrize("scene,accel,n,rpb,w,h,fs,ns", INPUT_CASES)
def test_inputs_equal_the_single_handle(T, sky, scene, accel, n, rpb, w, h, fs, ns):
    """After 1, 2 and 3 dispatches: both guide planes, the moments and the counts, as gathered from the members."""
    got = run(T, sky, n, rpb, w, h, scene, accel, fs, ns, 5)
    want = run(T, sky, 0, 0, w, h, scene, accel, fs, ns, 5)
    same_inputs(got, want, (scene, accel, n, rpb))
    assert got[-1]["inputs"]["T"] == DISPATCHES and got[-1]["inputs"]["P"] == DISPATCHES * ns
    last = want[-1]["inputs"]  # (and the planes hold something: hits, distances, albedo, luminance)
    assert last["albedo_hits"][..., 3].max() == DISPATCHES * min(fs, ns) and last["normal_depth"][..., 3].max() > 0
    assert last["albedo_hits"][..., :3].max() > 0 and last["moments"].max() > 0


@pytest.mark.parametrize("n,rpb,w,h", [GRID[1]])
def test_inputs_through_sample_batches(T, sky, n, rpb, w, h):
    """A radiance budget of two samples of the LARGEST member: 4 samples are 2 batches there, more on the single handle (its
    budget holds fewer samples of the whole frame) -- the moments go through `running` on both, in sample order."""
    lib = T.load_library()
    most = max(lib.srt_partition_owned_rows(h, r, n, rpb) for r in range(n)) * w
    budget = 2 * 12 * most
    assert budget < 4 * 12 * most and budget < 4 * 12 * w * h  # several batches on the members and on the reference
    got = run(T, sky, n, rpb, w, h, "mixed", 0, 3, 4, 5, budget=budget)
    want = run(T, sky, 0, 0, w, h, "mixed", 0, 3, 4, 5, budget=budget)
    same_inputs(got, want, ("batches", n, rpb))
    for g, s in zip(got, want):
        assert bits_equal(g["canvas"], s["canvas"]) and np.array_equal(g["bytes"], s["bytes"])
    whole = run(T, sky, 0, 0, w, h, "mixed", 0, 3, 4, 5)  # (and batches change nothing: the one-launch frame's inputs)
    same_inputs(got, whole, ("one launch", n, rpb))


# ---- 2. the filter -----------------------------------------------------------------------------------------------------------
FILTER_CASES = [(K, *SCENES[(g + k) % len(SCENES)], *GRID[g], *FS_NS[(g + 2 * ((g + k) % len(SCENES))) % len(FS_NS)])
                for k, K in enumerate((5, 0, 1)) for g in range(len(GRID))]


@pytest.mark.parametrize("K,scene,accel,n,rpb,w,h,fs,ns", FILTER_CASES)
def test_filtered_frames_equal_the_single_handle(T, sky, K, scene, accel, n, rpb, w, h, fs, ns):
    """render()'s bytes and read_denoised() for K = 0, 1, 5 a-trous passes; the canvas is the undenoised group's, and K = 0
    gives the bytes of the group with the denoiser off."""
    got = run(T, sky, n, rpb, w, h, scene, accel, fs, ns, K)
    want = run(T, sky, 0, 0, w, h, scene, accel, fs, ns, K)
    plain = run(T, sky, n, rpb, w, h, scene, accel, fs, ns, None)
    for d in range(DISPATCHES):
        assert np.array_equal(got[d]["bytes"], want[d]["bytes"]), (d, "bytes")
        assert bits_equal(got[d]["denoised"], want[d]["denoised"]), (d, "denoised")
        assert bits_equal(got[d]["canvas"], plain[d]["canvas"]), (d, "canvas")
        if K == 0:
            assert np.array_equal(got[d]["bytes"], plain[d]["bytes"]), (d, "K = 0")
    if K == 5:
        # (the filter did something; the last dispatch: after one dispatch of ONE sample the variance estimate is zero and the
        # luminance weight lets nothing through)
        assert not np.array_equal(got[-1]["bytes"], plain[-1]["bytes"])


# ---- 3. a group of one device: ncclCommInitAll / ncclGather ------------------------------------------------------------------
def frames(t, count, kind="move", first_time=900):
    """the front-end's loop with a moving camera: clear, update_scene, move, render; per frame the bytes and the filtered image"""
    out = []
    for k in range(count):
        t.clear_canvas()
        t.update_scene(*t.scene)
        t.options["camera_to_world"] = cam_at(k, kind)
        t.options["time"] = np.uint32(first_time + 17 * k)
        out.append((t.render(1).copy(), t.read_denoised()))
    return out


def same_frames(got, want, what):
    for k, (g, s) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], s[0]), (what, k, "bytes")
        assert bits_equal(g[1], s[1]), (what, k, "denoised")


def same_history(g, s, what):
    assert g["valid"] == s["valid"], what
    for k in ("colour", "count", "m1", "m2", "guide"):
        assert bits_equal(np.ascontiguousarray(g[k]), np.ascontiguousarray(s[k])), (what, k)
    assert g["camera"].tobytes() == s["camera"].tobytes(), what


def test_group_of_one_device_with_temporal(T, sky):
    w, h = 64, 40
    ts = [build(T, sky, n, 8, w, h, "mixed", 0, 2, virtual=False) for n in (0, 1)]  # the group: the real communicator and ncclGather
    for t in ts:
        t.set_denoise(feature_samples=2)
        t.set_denoise_temporal()
    single, group = ts
    same_frames(frames(group, 4), frames(single, 4), "one device")
    for k in INPUT_KEYS:
        assert bits_equal(group.read_denoise_inputs()[k], single.read_denoise_inputs()[k]), k
    group.clear_canvas(), single.clear_canvas()
    same_history(group.read_denoise_history(), single.read_denoise_history(), "one device")
    single.close(), group.close()


# ---- 4. temporal reprojection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,accel", [("spheres", 0), ("mesh_flat", 1)])
@pytest.mark.parametrize("n,rpb", [(3, 5), (8, 8)])
def test_moving_camera_sequence_equals_the_single_handle(T, sky, scene, accel, n, rpb):
    """8 frames render / clear / move: every frame's bytes and filtered image, then the history the last clear commits."""
    w, h = 64, 40
    ts = [build(T, sky, k, rpb, w, h, scene, accel, 2) for k in (0, n)]
    for t in ts:
        t.set_denoise()
        t.set_denoise_temporal(history_limit=6)
    single, group = ts
    got, want = frames(group, 8), frames(single, 8)
    same_frames(got, want, (scene, n, rpb))
    assert not np.array_equal(want[7][0], want[0][0])
    group.clear_canvas(), single.clear_canvas()
    hist = single.read_denoise_history()
    assert hist["valid"] and hist["count"].max() == 6.0  # (the sequence did integrate: the count reached the limit)
    same_history(group.read_denoise_history(), hist, (scene, n, rpb))
    single.close(), group.close()


def test_history_drops_like_the_single_handle(T, sky):
    """After each history-dropping call the next frame is the spatial-only frame -- on the group as on the single handle,
    whose frames the group's equal throughout."""
    w, h, n, rpb = 64, 40, 3, 5
    shapes, tris, mats = S.sphere_scene()
    moved = shapes.copy()
    moved["sphere_position"][0, 0] += 0.25
    tex = [np.full((2, 2, 4), 0.5, np.float32)]
    triggers = [("reset", lambda t: t.reset_denoise_history()), ("skybox", lambda t: t.set_skybox(sky)),
                ("textures", lambda t: t.set_textures(tex)), ("scene", lambda t: t.update_scene(moved, tris, mats)),
                ("temporal off/on", lambda t: (t.set_denoise_temporal(False), t.set_denoise_temporal()))]

    def sequence(t, spatial):
        """per trigger: a frame that commits a history, the trigger, the next frame (same camera and seed in `spatial`)"""
        out = []
        for i, (name, trig) in enumerate(triggers):
            t.scene = (shapes, tris, mats)
            pair = frames(t, 2, first_time=1000 + 100 * i)  # the second of these has a history
            t.clear_canvas()  # ... and becomes one
            assert t.read_denoise_history()["valid"], name
            trig(t)
            assert not t.read_denoise_history()["valid"], name
            if name == "scene":
                t.scene = spatial.scene = (moved, tris, mats)
            t.update_scene(*t.scene)
            t.options["camera_to_world"] = cam_at(2, "move")
            t.options["time"] = np.uint32(5000 + i)
            after = (t.render(1).copy(), t.read_denoised())
            spatial.clear_canvas()
            spatial.update_scene(*spatial.scene)
            spatial.options = t.options.copy()
            only = (spatial.render(1).copy(), spatial.read_denoised())
            assert np.array_equal(after[0], only[0]) and bits_equal(after[1], only[1]), name
            spatial.scene = (shapes, tris, mats)
            out += pair + [after]
        return out

    results = []
    for k in (0, n):
        t, spatial = build(T, sky, k, rpb, w, h, "spheres", 0, 2), build(T, sky, k, rpb, w, h, "spheres", 0, 2)
        t.set_denoise(), spatial.set_denoise()
        t.set_denoise_temporal()
        results.append(sequence(t, spatial))
        t.close(), spatial.close()
    assert len(results[0]) == 3 * len(triggers)
    same_frames(results[1], results[0], "drops")


# ---- 5. textures: the partition-aware textured feature kernels ---------------------------------------------------------------
def test_textured_scene_equals_the_single_handle(T, sky):
    w, h, n, rpb = 61, 29, 3, 2
    shapes, tris, mats, textures, bindings = S.textured_sphere_scene()
    recs = []
    for k in (0, n):
        t = T.Tracer(w, h) if k == 0 else T.TracerGroup(w, h, n_devices=n, devices=[0] * n, rows_per_block=rpb)
        t.set_skybox(sky)
        t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera(), time=4242)
        t.scene_data = R.scene_data(len(shapes))
        t.set_textures(textures)
        t.set_material_textures(bindings)
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        t.set_denoise(feature_samples=2)
        recs.append((t.render(1).copy(), t.read_denoised(), t.read_denoise_inputs()))
        t.close()
    (sb, sd, si), (gb, gd, gi) = recs
    assert np.array_equal(gb, sb) and bits_equal(gd, sd)
    for k in INPUT_KEYS:
        assert bits_equal(gi[k], si[k]), k
    untextured = run(T, sky, 0, 0, w, h, "spheres", 0, 2, 2, 5)  # (the texels are in the albedo plane)
    assert not bits_equal(si["albedo_hits"], untextured[0]["inputs"]["albedo_hits"])


# ---- 6. switches and errors --------------------------------------------------------------------------------------------------
def test_off_restores_the_plain_group(T, sky):
    n, rpb, w, h = GRID[1]
    plain = run(T, sky, n, rpb, w, h, "mixed", 0, 1, 2, None)
    g = build(T, sky, n, rpb, w, h, "mixed", 0, 2)
    g.set_denoise()
    g.set_denoise_temporal()
    g.options["time"] = np.uint32(5)
    g.render(1)
    g.set_denoise(False)  # keeps what is accumulated, as on a single handle: the caller clears
    g.clear_canvas()
    for d in range(DISPATCHES):
        g.options["time"] = np.uint32(777 + 31 * d)
        assert np.array_equal(g.render(d + 1), plain[d]["bytes"]), d
        assert bits_equal(g.read_canvas(), plain[d]["canvas"]), d
    # on again: cleared, and the single handle's frames again
    g.set_denoise(iterations=5, feature_samples=1)
    want = run(T, sky, 0, 0, w, h, "mixed", 0, 1, 2, 5)
    for d in range(DISPATCHES):
        g.options["time"] = np.uint32(777 + 31 * d)
        assert np.array_equal(g.render(d + 1), want[d]["bytes"]), d
        assert bits_equal(g.read_denoised(), want[d]["denoised"]), d
    g.close()


def test_off_keeps_the_accumulated_canvas(T, sky):
    """srt_set_denoise(NULL) does not clear: the samples on the canvas stay, on the group as on the single handle."""
    n, rpb, w, h = GRID[2]
    outs = []
    for k in (0, n):
        t = build(T, sky, k, rpb, w, h, "spheres", 0, 2)
        t.set_denoise()
        t.render(1)
        t.set_denoise(False)
        t.options["time"] = np.uint32(778)
        outs.append((t.render(2).copy(), t.read_canvas()))
        t.close()
    assert np.array_equal(outs[1][0], outs[0][0]) and bits_equal(outs[1][1], outs[0][1])


def test_error_codes(T, sky):
    lib = T.load_library()
    n, rpb, w, h = GRID[0]
    g = build(T, sky, n, rpb, w, h, "spheres", 0, 1)
    d, tp = T.DenoiseParams(), T.TemporalParams()
    assert lib.srt_denoise_defaults(C.byref(d)) == 0 and lib.srt_temporal_defaults(C.byref(tp)) == 0
    assert lib.srt_group_read_denoise_inputs(g._g, None, None, None, None) == 3  # never enabled
    assert lib.srt_group_read_denoise_history(g._g, None, None, None, None, None) == 3
    assert lib.srt_group_resolve_denoised(g._g, 1) == 3  # off
    assert lib.srt_group_set_denoise_temporal(g._g, None) == 0
    assert lib.srt_group_set_denoise_temporal(g._g, C.byref(tp)) == 3  # the denoiser is off
    for field, bad in [("iterations", -1), ("iterations", 9), ("feature_samples", 0), ("feature_samples", 65), ("sigma_luminance", 0.0),
                       ("sigma_normal", float("nan")), ("sigma_depth", float("inf")), ("sigma_albedo", -1.0), ("reserved", 1)]:
        e = T.DenoiseParams.from_buffer_copy(d)
        setattr(e, field, bad)
        assert lib.srt_group_set_denoise(g._g, C.byref(e)) == 1, field
    assert lib.srt_group_resolve_denoised(g._g, 1) == 3  # a refused call left it off
    assert lib.srt_group_set_denoise(g._g, C.byref(d)) == 0
    assert lib.srt_group_resolve_denoised(g._g, 1) == 3  # nothing traced since the clear
    with pytest.raises(T.SrtError):
        g.read_denoised()  # no filtered image yet
    for field, bad in [("history_limit", 0), ("normal_threshold", 1.5), ("depth_threshold", 0.0)]:
        e = T.TemporalParams.from_buffer_copy(tp)
        setattr(e, field, bad)
        assert lib.srt_group_set_denoise_temporal(g._g, C.byref(e)) == 1, field
    assert lib.srt_group_set_denoise_temporal(g._g, C.byref(tp)) == 0
    # the per-handle rules stand on a member
    member = g.member(1)
    assert lib.srt_set_denoise(member, C.byref(d)) == 3
    assert lib.srt_set_denoise_temporal(member, C.byref(tp)) == 3
    assert lib.srt_set_partition(member, 1, n, rpb) == 3 and lib.srt_bind_canvas(member, None, 0) == 3  # the group's denoiser is on
    g.render(1)
    g.trace_and_gather()
    g.resolve_denoised(2)
    assert g.read_denoise_inputs()["T"] == 2
    assert lib.srt_group_set_denoise(g._g, None) == 0
    assert lib.srt_set_denoise(member, C.byref(d)) == 3  # still a partitioned handle
    assert lib.srt_set_partition(member, 1, n, rpb) == 0
    assert lib.srt_group_read_denoised(g._g, None) == 1
    g.close()


# ---- 7. the multi-plane unpermute kernel alone ---------------------------------------------------------------------------------
def test_unpermute_planes_kernel_on_a_hand_packed_three_rank_buffer(T):
    """Values encode (plane, rank, packed row, x, channel); padding rows and the moments plane's padding hold values too,
    which must not show up anywhere in the image. 37 rows in blocks of 3 over 3 ranks: a last block of one row, a last
    round of one block; 41 x 15 pixels per plane is no multiple of four, so the slots are padded."""
    import torch
    lib = T.load_library()
    w, h, world, rpb = 41, 37, 3, 3
    padded = T.padded_rows(h, world, rpb)
    plane = padded * w
    slot = lib.srt_partition_planes_floats(w, h, world, rpb)
    assert slot == 12 * plane + (plane + 3) // 4 * 4 and plane % 4 != 0
    assert lib.srt_partition_planes_floats(0, h, world, rpb) == -1

    def code(p, r, lr, x, c):
        return np.float32(((((p * 4 + r) * 64 + lr) * 64 + x) * 4 + c) + 1)

    packed = np.full((world, slot), -7.0, np.float32)  # (-7: the slot padding)
    lr, x, c = np.meshgrid(np.arange(padded), np.arange(w), np.arange(4), indexing="ij")
    for r in range(world):
        for p in range(3):
            packed[r, 4 * plane * p:4 * plane * (p + 1)] = code(p, r, lr, x, c).ravel()
        packed[r, 12 * plane:13 * plane] = code(3, r, lr[..., 0], x[..., 0], 0).ravel()
    want = [np.zeros((h, w, 4), np.float32) for _ in range(3)] + [np.zeros((h, w), np.float32)]
    seen = 0
    for r in range(world):
        for row in range(padded):
            y = T.global_row(h, r, world, rpb, row)
            if y < 0:
                continue  # padding: its codes appear nowhere below
            seen += 1
            for p in range(3):
                want[p][y] = code(p, r, row, x[0], c[0])
            want[3][y] = code(3, r, row, x[0, :, 0], 0)
    assert seen == h
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(packed).to(dev)
    outs = [torch.full(a.shape, -1.0, dtype=torch.float32, device=dev) for a in want]
    assert lib.srt_unpermute_planes_device(*(C.c_void_p(o.data_ptr()) for o in [src] + outs), w, h, world, rpb) == 0
    torch.cuda.synchronize()
    for p, (o, a) in enumerate(zip(outs, want)):
        assert np.array_equal(o.cpu().numpy(), a), p
    assert lib.srt_unpermute_planes_device(None, None, None, None, None, w, h, world, rpb) == 1


# ---- 8. srt_headless --gpus N --denoise K --temporal ---------------------------------------------------------------------------
def test_headless_group_writes_the_single_device_frames(T, tmp_path):
    from simple_raytracer_amd import build as B
    exe = B.build_headless()
    outs = []
    for gpus in (1, 4):  # 4 on this box's one GPU: virtual devices
        ppm = tmp_path / f"g{gpus}.ppm"
        subprocess.run([str(exe), "--scene", "spheres", "--width", "64", "--height", "40", "--spp", "2", "--frames", "3", "--denoise", "5",
                        "--temporal", "--move", "0.02", "--gpus", str(gpus), "--out", str(ppm)], check=True, timeout=120)
        outs.append(ppm.read_bytes())
    assert len(outs[0]) > 64 * 40 * 3 and outs[1] == outs[0]
