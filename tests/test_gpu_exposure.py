"""GPU: exposure for the resolve (include/srt_abi.h srt_set_exposure; csrc/exposure.hip) against tests/exposure_ref.py.

  histogram  hist and counts of read_exposure() equal the reference's integer for integer, on frames of 1x1, 7x5 (less than a
             wave), 64x4 (one workgroup), 257x3 (a ragged last workgroup) and 513x512: srt_exposure_hist_kernel runs at most
             SRT_EX_HIST_GRID_CAP = 1024 workgroups of 256 lanes (csrc/exposure.hip), 262144 lanes, so the 262656 pixels of the
             last frame make the first 512 lanes stride
  scalar     log2_exposure and exposure within 2 float ulps of the reference's float64 result rounded to float (at most 256
             double additions and one double exp2 keep the device value far inside half a float ulp of the reference's, so
             the two roundings differ by at most 1 ulp; doubled for margin)
  bytes      the ARGB bytes equal the reference's computed from the canvas and the exposure read back from the device, bit for
             bit, on the byte-boundary canvases of tests/tonemap_cases.py
  sites      every resolving call gives the same exposed bytes for the same frame

Planted canvases are bound device tensors, as in tests/test_gpu_tonemap_edges.py; they only need srt_resolve, not a trace."""
import functools

import numpy as np
import pytest

import exposure_ref as E
import tonemap_cases as TC
from gpu_harness import T, make  # noqa: F401 (T: the fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
HIST_GRID_CAP = 1024  # csrc/exposure.hip SRT_EX_HIST_GRID_CAP
FRAMES = [(1, 1), (7, 5), (64, 4), (257, 3), (513, 512)]
assert FRAMES[-1][0] * FRAMES[-1][1] > HIST_GRID_CAP * 256 > FRAMES[-2][0] * FRAMES[-2][1]
CONTENTS = ["one_luminance", "log_uniform", "specials", "bin_edges"]


def grey(v):
    v = np.asarray(v, F32)
    return np.stack([v, v, v, np.full_like(v, np.nan)], axis=-1)  # alpha: garbage that must never be read


@functools.lru_cache(maxsize=None)
def edge_pixels():
    """Pixels (x, x, y, NaN) whose luminance (the reference's float32 expression) is exactly a bin edge, and ones whose
    luminance is the largest float below one: found by search among the x and y within 8 ulps of each edge.
    -> (on, below), (k, 4) float32 each, one pixel per edge that has one."""
    b = np.arange(1, E.BINS)
    edge = (np.ldexp(1.0, b // 4 - 32) * (1.0 + (b % 4) / 4.0)).astype(F32)
    near = (edge.view(np.uint32).astype(np.int64)[:, None] + np.arange(-8, 9)[None, :]).astype(np.uint32).view(F32)  # (255, 17)
    px = np.empty((len(b), 17, 17, 4), F32)
    px[..., 0] = px[..., 1] = near[:, :, None]
    px[..., 2] = near[:, None, :]
    px[..., 3] = np.nan  # alpha: garbage that must never be read
    L = E.luminance(px.reshape(-1, 4), 1).reshape(len(b), -1)
    px = px.reshape(len(b), -1, 4)
    on = [p[l == e][:1] for p, l, e in zip(px, L, edge)]
    below = [p[l == np.nextafter(e, F32(0))][:1] for p, l, e in zip(px, L, edge)]
    on, below = np.concatenate(on), np.concatenate(below)
    assert len(on) >= 250 and len(below) >= 250, (len(on), len(below))
    return on, below


@functools.lru_cache(maxsize=None)
def content(name, n):
    """(n, 4) float32 canvas pixels and the ticks they are resolved with."""
    rng = np.random.RandomState(n * 7 + len(name))
    if name == "one_luminance":
        return grey(np.full(n, 0.37, F32)), 1
    if name == "log_uniform":  # luminances over 40 octaves, random chroma, divided by 3 on the device
        L = np.exp2(rng.uniform(-20, 20, n))
        px = grey(np.ones(n, F32))
        px[:, :3] = (L[:, None] * rng.uniform(0.2, 3.0, (n, 3)) * 3.0).astype(F32)
        return px, 3
    if name == "specials":  # 0, -1, +inf, NaN: left out; a denormal: bin 0; the rest ordinary
        v = np.exp2(rng.uniform(-6, 6, n)).astype(F32)
        special = np.array([0.0, -1.0, np.inf, np.nan, 1e-40, -0.0, -np.inf], F32)
        at = np.arange(len(special)) * max(1, n // 11) % n if n >= len(special) else np.arange(n)
        v[at[:n]] = special[:n]
        return grey(v), 1
    on, below = edge_pixels()
    v = np.concatenate([on, below, grey([F32(2.0 ** -33), F32(2.0 ** 33)])])
    return v[np.resize(rng.permutation(len(v)), n)], 1


def planted(T, w, h, pixels):
    """A Tracer of w x h whose bound canvas holds `pixels`; -> tracer, the device tensor (kept alive by the caller)."""
    import torch
    t = T.Tracer(w, h)
    c = torch.from_numpy(np.array(pixels, F32).reshape(h, w, 4)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    t.bind_canvas(c.data_ptr(), c.numel() * 4)
    return t, c


def refill(t, c, pixels):
    import torch
    t.synchronize()
    c.copy_(torch.from_numpy(np.ascontiguousarray(pixels, F32).reshape(tuple(c.shape))))
    torch.cuda.synchronize()


def done(t):
    t.bind_canvas(0, 0)
    t.close()


def check_scalar(got, want, what):
    for k, name in enumerate(("log2_exposure", "exposure")):
        d = E.ulps(got[name], want[k])
        print(f"{what}: {name} device {got[name]!r} reference {want[k]!r} ({d} ulps)")
        assert d <= 2, (what, name, got[name], want[k])


@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("w,h", FRAMES, ids=lambda v: str(v))
def test_histogram_is_exact(T, w, h, name):
    px, ticks = content(name, w * h)
    t, c = planted(T, w, h, px)
    t.set_exposure(mode="auto")
    t.resolve(ticks)
    got = t.read_exposure()
    hist, counts = E.histogram(px, ticks)
    assert (got["metered"], got["left_out"]) == counts and counts[0] + counts[1] == w * h
    assert np.array_equal(got["hist"], hist)
    if name == "specials" and w * h >= 7:
        assert counts[1] == 6 and hist[0] >= 1  # 0, -1, +inf, NaN, -0, -inf left out; the denormal metered
    if name == "bin_edges" and w * h >= 1000:
        assert np.count_nonzero(hist) >= 250 and hist[0] >= 1 and hist[255] >= 1
    check_scalar(got, E.Meter().frame(hist), (w, h, name))
    assert t.last_resolve_exposed()
    assert np.array_equal(t.read_argb().reshape(-1, 4), E.exposed_bytes(px, ticks, got["exposure"]))
    done(t)


@pytest.mark.parametrize("params", [dict(low_permille=0, high_permille=1000), dict(low_permille=100, high_permille=950),
                                    dict(low_permille=500, high_permille=501), dict(low_permille=999, high_permille=1000, ev=1.5, key=0.5)], ids=str)
def test_exposure_scalar_over_windows(T, params):
    w, h = 257, 3
    px, ticks = content("log_uniform", w * h)
    hist, _ = E.histogram(px, ticks)
    if params["high_permille"] - params["low_permille"] == 1:  # the window lies inside one bin
        lo, hi = E.window(w * h, params["low_permille"], params["high_permille"])
        cum = np.cumsum(hist.astype(np.int64))
        assert hi == lo + 1 and np.searchsorted(cum, lo, side="right") == np.searchsorted(cum, hi - 1, side="right")
    t, c = planted(T, w, h, px)
    t.set_exposure(mode="auto", **params)
    t.resolve(ticks)
    check_scalar(t.read_exposure(), E.Meter(**params).frame(hist), params)
    done(t)


def test_clamp_zero_pixels_adaptation_and_reset(T):
    w, h = 64, 4
    dim, bright, black = grey(np.full(w * h, 1.0, F32)), grey(np.full(w * h, 16.0, F32)), grey(np.zeros(w * h, F32))
    H = {k: E.histogram(v, 1)[0] for k, v in (("dim", dim), ("bright", bright), ("black", black))}
    assert H["black"].sum() == 0 and H["dim"][128] == w * h
    t, c = planted(T, w, h, black)

    def frame(pixels, meter, what, hist):
        refill(t, c, pixels)
        t.resolve(1)
        got = t.read_exposure()
        check_scalar(got, meter.frame(hist), what)
        return got

    # a fresh handle that meters nothing: state 0, the bias alone -- and that frame is no state to adapt from
    m = E.Meter(ev=0.75, adapt=0.25)
    t.set_exposure(mode="auto", ev=0.75, adapt=0.25)
    got = frame(black, m, "fresh, nothing metered", H["black"])
    assert got["log2_exposure"] == F32(0.75) and (got["metered"], got["left_out"]) == (0, w * h)
    first = frame(dim, m, "first metered frame adopts its target", H["dim"])
    assert E.ulps(first["log2_exposure"], F32(np.log2(np.float64(F32(0.18))) - 0.125 + 0.75)) <= 2
    # a step change, five frames at adapt = 0.25
    seq = [frame(bright, m, f"step {k}", H["bright"])["log2_exposure"] for k in range(5)]
    assert all(a > b for a, b in zip([first["log2_exposure"]] + seq, seq))
    # nothing metered keeps the state; srt_clear_canvas keeps it too
    kept = frame(black, m, "nothing metered keeps the state", H["black"])
    assert kept["log2_exposure"] == seq[-1]
    t.clear_canvas()
    t.synchronize()
    # reset: the next frame adopts its target
    t.reset_exposure()
    m.reset()
    again = frame(dim, m, "after reset", H["dim"])
    assert again["log2_exposure"] == first["log2_exposure"]
    # disabling forgets the state as well
    frame(bright, m, "one step", H["bright"])
    t.set_exposure(False)
    m.reset()
    for params, want in ((dict(min_ev=-1.0), -1.0), (dict(max_ev=-4.0), -4.0), (dict(min_ev=-2.5, max_ev=-2.5, ev=-1.0), -3.5)):
        t.set_exposure(mode="auto", **params)
        t.reset_exposure()
        got = frame(dim, E.Meter(**params), params, H["dim"])
        assert got["log2_exposure"] == F32(want)
    done(t)


@pytest.mark.parametrize("mode", ["manual", "auto"])
@pytest.mark.parametrize("scale", [2.0 ** -3, 1.0, 2.0 ** 5], ids=["2^-3", "1", "2^5"])
def test_bytes_are_exact_on_the_byte_boundary_canvases(T, scale, mode):
    """tonemap(c * e) on values that land on and around every byte boundary after the multiplication: the crafted canvas scaled
    by 1 / e for MANUAL e = 2^3, 1, 2^-5 (exact scalings), and as it is for AUTO, where e is whatever the meter gives."""
    with np.errstate(all="ignore"):
        crafted = (TC.natural_image() * F32(scale)).astype(F32)
    h, w = crafted.shape[:2]
    t, c = planted(T, w, h, crafted)
    if mode == "manual":
        t.set_exposure(mode="manual", ev=-np.log2(scale))
    else:
        t.set_exposure(mode="auto")
    m = E.Meter()
    for ticks in TC.TICKS:
        t.resolve(ticks)
        got = t.read_exposure()
        if mode == "manual":
            assert (got["log2_exposure"], got["exposure"]) == E.manual(-np.log2(scale))
            assert got["metered"] == 0
        else:
            hist, counts = E.histogram(crafted, ticks)
            assert np.array_equal(got["hist"], hist) and (got["metered"], got["left_out"]) == counts
            check_scalar(got, m.frame(hist), (scale, ticks))  # (ticks 0: nothing metered, the state of the frame before)
        assert t.last_resolve_exposed()
        assert np.array_equal(t.read_argb().reshape(-1, 4), E.exposed_bytes(crafted, ticks, got["exposure"])), (scale, mode, ticks)
    if mode == "manual":  # the scaled canvas times e is the crafted one: the plain resolve's bytes of that, every boundary met
        t.resolve(1)
        assert np.array_equal(t.read_argb().reshape(-1, 4), E.exposed_bytes(TC.natural_image(), 1, 1.0))
    done(t)


def test_exposed_resolve_past_its_grid_cap(T):
    """srt_exposure_resolve_kernel runs at most 4096 workgroups, as srt_resolve_kernel: 4096 * 256 + 257 pixels make its lanes
    stride (and the histogram's eight times over)."""
    px = TC.pixels(TC.LARGE_PIXELS)
    t, c = planted(T, TC.LARGE_PIXELS, 1, px)
    t.set_exposure(mode="auto", ev=0.5)
    t.resolve(3)
    got = t.read_exposure()
    hist, counts = E.histogram(px, 3)
    assert np.array_equal(got["hist"], hist) and (got["metered"], got["left_out"]) == counts
    check_scalar(got, E.Meter(ev=0.5).frame(hist), "large")
    assert np.array_equal(t.read_argb().reshape(-1, 4), E.exposed_bytes(px, 3, got["exposure"]))
    done(t)


def test_off_and_identity(T):
    crafted = TC.natural_image()
    h, w = crafted.shape[:2]
    t, c = planted(T, w, h, crafted)
    plain = {}
    for ticks in TC.TICKS:
        t.resolve(ticks)
        plain[ticks] = t.read_argb().copy()
        assert not t.last_resolve_exposed()
    never = t.read_exposure()
    assert (never["log2_exposure"], never["exposure"], never["metered"], never["left_out"]) == (0, 1, 0, 0) and not never["hist"].any()
    t.set_exposure(mode="manual", ev=0.0)
    for ticks in TC.TICKS:
        t.resolve(ticks)
        assert t.last_resolve_exposed()
        assert np.array_equal(t.read_argb(), plain[ticks]), ticks
    t.set_exposure(mode="manual", ev=2.0)
    t.resolve(1)
    assert t.last_resolve_exposed() and not np.array_equal(t.read_argb(), plain[1])
    t.set_exposure(False)
    assert not t.last_resolve_exposed()
    for ticks in TC.TICKS:
        t.resolve(ticks)
        assert not t.last_resolve_exposed()
        assert np.array_equal(t.read_argb(), plain[ticks]), ticks
    # srt_resolve_external keeps the plain bytes with the feature on
    import torch
    t.set_exposure(mode="manual", ev=2.0)
    argb = torch.zeros((h * w, 4), dtype=torch.uint8, device=c.device)
    t.resolve_external(c.data_ptr(), h * w, 1, argb.data_ptr())
    t.synchronize()
    assert np.array_equal(argb.cpu().numpy().reshape(plain[1].shape), plain[1])
    with pytest.raises(T.SrtError):
        t.set_exposure(mode="auto", adapt=0.0)
    done(t)


W, H, SPP = 48, 32, 2
PARAMS = dict(mode="auto", ev=0.25, low_permille=50, high_permille=900)


def test_every_site_gives_the_same_exposed_bytes(T, sky):
    t = make(T, sky, "spheres", W, H, spp=SPP)
    t.render(1)
    canvas, plain = t.read_canvas(), t.read_argb().copy()
    hist, _ = E.histogram(canvas, 1)
    l2, e = E.Meter(**{k: v for k, v in PARAMS.items() if k != "mode"}).frame(hist)
    t.set_exposure(**PARAMS)
    out = {}

    def fresh():
        t.clear_canvas()
        t.reset_exposure()

    fresh()
    out["render"] = t.render(1).copy()
    assert t.last_resolve_exposed()
    got = t.read_exposure()
    check_scalar(got, (l2, e), "render")
    assert np.array_equal(got["hist"], hist)
    want = E.exposed_bytes(canvas, 1, got["exposure"])
    assert not np.array_equal(want, plain.reshape(-1, 4))  # the exposure changes this frame's bytes
    fresh()
    t.trace()
    t.resolve(1)
    out["trace + resolve"] = t.read_argb().copy()
    assert t.last_resolve_exposed()
    fresh()
    buf = np.zeros(W * H * 4, np.uint8)
    t.render_async(1, buf)
    t.synchronize()
    out["render_async"] = buf.copy()
    assert t.last_resolve_exposed()
    fresh()
    buf2 = np.zeros(W * H * 4, np.uint8)
    assert t.render_pipelined(1, buf2) == -1
    assert t.pipeline_flush(buf2) == 0
    out["render_pipelined"] = buf2.copy()
    assert t.last_resolve_exposed()
    assert np.array_equal(t.read_canvas().view(np.uint32), canvas.view(np.uint32))
    t.close()
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
    g.set_skybox(sky)
    g.options, g.scene_data = t.options.copy(), t.scene_data.copy()
    g.update_scene(*t.scene)
    g.clear_canvas()
    assert not g.last_resolve_exposed()
    g.set_exposure(**PARAMS)
    out["group"] = g.render(1).copy()
    assert g.last_resolve_exposed()
    assert np.array_equal(g.read_canvas().view(np.uint32), canvas.view(np.uint32))
    gx = g.read_exposure()
    assert (gx["log2_exposure"], gx["exposure"]) == (got["log2_exposure"], got["exposure"]) and np.array_equal(gx["hist"], hist)
    g.close()
    for site, b in out.items():
        assert np.array_equal(b.reshape(-1, 4), want), site


@pytest.mark.parametrize("group", [False, True], ids=["handle", "group"])
def test_denoised_resolve_exposes_the_filtered_image(T, sky, group):
    if group:
        t = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
        t.set_skybox(sky)
        ref = make(T, sky, "spheres", W, H, spp=SPP)
        t.options, t.scene_data = ref.options.copy(), ref.scene_data.copy()
        t.update_scene(*ref.scene)
        ref.close()
        t.clear_canvas()
        t.set_denoise(iterations=2)
    else:
        t = make(T, sky, "spheres", W, H, spp=SPP, denoise=dict(iterations=2))
    t.set_exposure(**PARAMS)
    if group:
        t.trace_and_gather()
    else:
        t.trace()
    t.resolve_denoised(1)
    assert t.last_resolve_exposed()
    hdr = t.read_denoised()
    got = t.read_exposure()
    hist, counts = E.histogram(hdr, None)
    assert np.array_equal(got["hist"], hist) and (got["metered"], got["left_out"]) == counts
    check_scalar(got, E.Meter(**{k: v for k, v in PARAMS.items() if k != "mode"}).frame(hist), "denoised")
    argb = t.read_argb() if not group else None
    if group:
        out = t.render(2)  # a second frame through srt_group_render's denoised branch
        assert t.last_resolve_exposed()
        hdr, got = t.read_denoised(), t.read_exposure()
        argb = out
    assert np.array_equal(np.asarray(argb).reshape(-1, 4), E.exposed_bytes(hdr, None, got["exposure"]))
    t.close()


def test_pipelined_frames_adapt_like_blocking_frames(T, sky):
    """Three frames accumulating on one canvas with adapt = 0.5: the bytes of every frame and the final exposure are the same
    whether the frames are rendered one by one or two deep, where nothing between frames waits for the device."""
    params = dict(mode="auto", adapt=0.5, ev=-0.5)
    runs = []
    for pipelined in (False, True):
        t = make(T, sky, "spheres", W, H, spp=SPP)
        t.set_exposure(**params)
        frames, bufs = [], [np.zeros(W * H * 4, np.uint8) for _ in range(4)]
        for k in range(3):
            t.options["time"] = np.uint32(777 + 31 * k)
            if pipelined:
                if t.render_pipelined(k + 1, bufs[k]) >= 0:
                    frames.append(bufs[k].copy())
            else:
                frames.append(t.render(k + 1).copy())
        if pipelined:
            t.synchronize()  # (both frames in flight are done; the flush hands out the newest)
            assert t.pipeline_flush(bufs[3]) == 2
            frames.append(bufs[3].copy())
        runs.append((frames, t.read_exposure(), t.read_canvas()))
        t.close()
    (fb, xb, cb), (fp, xp, cp) = runs
    assert np.array_equal(cb.view(np.uint32), cp.view(np.uint32))
    assert (xb["log2_exposure"], xb["exposure"]) == (xp["log2_exposure"], xp["exposure"]) and np.array_equal(xb["hist"], xp["hist"])
    assert len(fb) == 3 and len(fp) == 3
    assert np.array_equal(fb[0], fp[0]) and np.array_equal(fb[1], fp[1]) and np.array_equal(fb[2], fp[2])
    # and the last frame's bytes are the reference's for the exposure the three-frame sequence ends on
    assert np.array_equal(fb[2].reshape(-1, 4), E.exposed_bytes(cb, 3, xb["exposure"]))
