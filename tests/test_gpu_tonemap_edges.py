"""GPU: every device site of canvas / ticks -> ACES fit -> sqrt -> * 255 -> truncate -> A, R, G, B, on the crafted canvas of
tests/tonemap_cases.py: values on and within 64 ulps of every place where a byte changes, values that land there after the
division by 3, 7, 10, 2^24 and 2^32, and the non-finite ends. Every comparison is exact.

The expression is written out three times in the device code; which test reaches which copy, with which inputs:

  srt_resolve_kernel (csrc/frame.hip)                    test_resolve_and_resolve_external: srt_resolve on handles of 1, 255, 257
                                                         and 211 x 259 pixels, srt_resolve_external on the same counts and on
                                                         4096 * 256 + 257 pixels (the grid-stride loop's second trip), every
                                                         ticks of tonemap_cases.TICKS, against oracle.average
  srt_reduce_kernel<false>'s fused resolve (frame.hip)   test_fused_resolve_of_render: srt_render of a scene whose radiance is
                                                         exactly +0 into the pre-filled bound canvas, 1 sample, 4 samples (the
                                                         float4 loads), 12 samples in three batches; every ticks
  tonemap() (csrc/tonemap.h) in
    srt_denoise_setup_kernel (csrc/denoise.hip)          test_denoiser_without_passes: iterations = 0, every ticks, against
                                                         denoise_ref.tonemap(canvas / ticks) and the plain resolve's bytes
    srt_denoise_atrous_kernel's last pass                test_filtered_bytes_are_the_tonemap_of_the_filtered_floats[plain-*]
    srt_denoise_atrous_demod_kernel<true>                ...[demod-*]
    srt_temporal_kernel<0, false, false> (csrc/temporal.hip)   ...[temporal-0]: iterations = 0 with a valid history

Sites that share one of these and are covered through it (read in csrc/srt_collect.hip, csrc/srt_group.hip, csrc/frame_pipeline.hip and csrc/srt_abi.hip):
srt_resolve_gathered calls srt_resolve_external; srt_group_render calls srt_resolve_gathered, or with the group's denoiser on
srt_resolve_denoised on its resolver handle (srt_denoise_filter, the kernels above); a group member's srt_render with the
group's denoiser on resolves through launch_resolve (srt_resolve_kernel); srt_render with the handle's denoiser on runs
srt_denoise_filter; srt_render_async and srt_render_pipelined run srt_trace_fused as srt_render does. None has an expression of
its own.
"""
import numpy as np
import pytest

import denoise_ref as D
import tonemap_cases as TC
from conftest import bits_equal
from gpu_harness import T, make  # noqa: F401 (T: the fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = (TC.natural_image().shape[0] * TC.WIDTH, 1, 255, 257)


def device_canvas(pixels):
    """A torch tensor (n, 4) float32 on the device holding `pixels`."""
    import torch
    c = torch.from_numpy(np.array(pixels, F32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return c


def fill(t, canvas, pixels):
    """Overwrite the bound canvas with `pixels` once the handle's stream is idle."""
    import torch
    t.synchronize()
    canvas.copy_(torch.from_numpy(np.array(pixels, F32).reshape(tuple(canvas.shape))))
    torch.cuda.synchronize()


def bind(t, pixels):
    """Bind a fresh device tensor (height, width, 4) as t's canvas; filled with `pixels` (zeros when None)."""
    c = device_canvas(np.zeros((t.height, t.width, 4), F32) if pixels is None else np.asarray(pixels, F32).reshape(t.height, t.width, 4))
    t.synchronize()
    t.bind_canvas(c.data_ptr(), c.numel() * 4)
    return c


def zero_tracer(T, sky, spp=1, **kw):
    """A Tracer of the natural image's size over tonemap_cases.zero_scene(), with a bound canvas of zeros."""
    h, w = TC.natural_image().shape[:2]
    t = make(T, sky, TC.zero_scene(), w, h, spp=spp, **kw)
    return t, bind(t, None)


@pytest.mark.parametrize("count", COUNTS + (TC.LARGE_PIXELS,))
def test_resolve_and_resolve_external(T, oracle, count):
    """srt_resolve_kernel: bytes == oracle.average(ticks, canvas) for every ticks, through srt_resolve on a handle of exactly
    `count` pixels (its own argb image) and through srt_resolve_external (a caller's); the large count, past the 4096-block
    grid cap, through srt_resolve_external alone."""
    import torch
    px = TC.pixels(count)
    large = count == TC.LARGE_PIXELS
    w, h = (TC.WIDTH, count // TC.WIDTH) if count == COUNTS[0] else (1, 1) if large else (count, 1)
    t = T.Tracer(w, h)
    canvas = device_canvas(px)
    if not large:
        t.bind_canvas(canvas.data_ptr(), canvas.numel() * 4)
    argb = torch.zeros((count, 4), dtype=torch.uint8, device=canvas.device)
    for ticks in TC.TICKS:
        want = oracle.average(ticks, px)
        argb.fill_(0x5A)
        torch.cuda.synchronize()
        t.resolve_external(canvas.data_ptr(), count, ticks, argb.data_ptr())
        t.synchronize()
        assert np.array_equal(argb.cpu().numpy(), want), (count, ticks, "external")
        if not large:
            t.resolve(ticks)
            assert np.array_equal(t.read_argb().reshape(-1, 4), want), (count, ticks)
    assert bits_equal(canvas.cpu().numpy(), px)  # the resolve only reads
    t.bind_canvas(0, 0)
    t.close()


@pytest.mark.parametrize("spp,fit", [(1, None), (4, None), (12, 8)])
def test_fused_resolve_of_render(T, sky, oracle, spp, fit):
    """srt_reduce_kernel<false>: srt_render adds the frame's colour, exactly +0 in this scene (tests/test_tonemap_cases.py checks
    that on the oracle), to the pre-filled bound canvas and resolves what it has just written. The canvas read back is the
    crafted one bit for bit but for -0, which -0 + 0 turns into +0, with every NaN still a NaN and the alpha lane untouched; the
    returned bytes are oracle.average(ticks, canvas read back). fit: a radiance budget of that many samples per pixel; the batches
    of a frame alternate between two buffers that both have to fit, so 12 samples run as three batches of 4 (a frame cannot be
    made to run as exactly two) and only the last reduction resolves."""
    t, canvas = zero_tracer(T, sky, spp=spp)
    crafted = TC.natural_image()
    if fit:
        t.set_radiance_budget(crafted.shape[0] * crafted.shape[1] * 12 * fit)
    for ticks in TC.TICKS:
        fill(t, canvas, crafted)
        out = t.render(ticks)
        assert t.last_trace_launches()[0] == (3 if fit else 1)
        back = canvas.cpu().numpy()
        assert TC.same_canvas(back, crafted), ticks
        assert np.array_equal(out.reshape(back.shape), oracle.average(ticks, back)), ticks
    assert t.counters()["nan_pixels"] == 0  # (counts the frame's own colour, not the canvas)
    t.bind_canvas(0, 0)
    t.close()


def test_denoiser_without_passes(T, sky):
    """srt_denoise_setup_kernel (iterations = 0): its bytes are denoise_ref.tonemap(canvas / ticks) and the plain srt_resolve's
    of the same canvas -- the two textual copies held equal --, and read_denoised() is canvas / ticks bit for bit."""
    t, canvas = zero_tracer(T, sky, denoise=dict(iterations=0))
    t.trace()  # something traced since the clear: srt_resolve_denoised accepts the call
    crafted = TC.natural_image()
    fill(t, canvas, crafted)
    for ticks in TC.TICKS:
        with np.errstate(all="ignore"):
            c0 = (crafted[..., :3] / TC.f32_ticks(ticks)).astype(F32)
        t.resolve_denoised(ticks)
        got = t.read_argb()
        assert np.array_equal(got, D.tonemap(c0)), ticks
        assert bits_equal(t.read_denoised()[..., :3], c0), ticks
        t.resolve(ticks)
        assert np.array_equal(t.read_argb(), got), ticks
    t.bind_canvas(0, 0)
    t.close()


@pytest.mark.parametrize("mode,iterations", [("plain", 1), ("plain", 3), ("demod", 1), ("demod", 2), ("temporal", 0)])
def test_filtered_bytes_are_the_tonemap_of_the_filtered_floats(T, sky, mode, iterations):
    """The passes' last launch and the temporal set-up change the values before they convert them, so no crafted value reaches
    the conversion untouched; the crafted canvas goes in as a dense ramp all the same and read_argb() must be
    denoise_ref.tonemap(read_denoised()) exactly, pixels whose filtered value is NaN or inf included.

    Coverage (a condition on the inputs, computed by the CPU reference from the floats read back; at least 1000 asked for):
    filtered channel values within 64 ulps of a byte boundary -- plain, 1 and 3 passes: 98569, 98528; demod, 1 and 2 passes:
    98450, 98406; temporal set-up: 98664; each of 163890 finite positive ones (the 3 x 32895 values of the boundary windows;
    the divided windows are undivided here). 15 channel values are not finite, 21 with demodulation or the doubling. The frame's
    variance is 0 (its moments are the zero scene's), so a tap of another luminance weighs exp(-1e10 |dl|) = 0 and a pixel
    keeps (w c) / w of its own value; demodulation divides by and multiplies with the albedo floor; the temporal set-up halves
    the canvas (one sample now, one of exactly 0 in the history), so it is fed twice the crafted values."""
    temporal = mode == "temporal"
    t, canvas = zero_tracer(T, sky, denoise=dict(iterations=iterations), temporal={} if temporal else None)
    if mode == "demod":
        t.set_denoise_demodulation(True)
    t.trace()
    crafted = TC.natural_image()
    if temporal:
        t.clear_canvas()  # the zero frame becomes the history
        assert t.read_denoise_history()["valid"]
        t.trace()
        with np.errstate(all="ignore"):
            crafted = (crafted * F32(2)).astype(F32)
    fill(t, canvas, crafted)
    t.resolve_denoised(1)
    hdr, argb = t.read_denoised(), t.read_argb()
    assert t.last_filter_demodulated() == (mode == "demod")
    assert np.array_equal(argb, D.tonemap(hdr[..., :3])), (mode, iterations)
    near, strange = TC.near_boundary(hdr[..., :3]), int(np.sum(~np.isfinite(hdr[..., :3])))
    print(f"{mode} {iterations}: {near} filtered values within {TC.WIDE} ulps of a boundary, {strange} not finite, "
          f"{int(np.sum(np.isfinite(hdr[..., :3]) & (hdr[..., :3] > 0)))} finite and positive")
    assert near >= 1000 and strange >= 15  # (three NaNs and +-inf in each of the three channels, at the least)
    t.bind_canvas(0, 0)
    t.close()
