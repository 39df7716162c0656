"""CPU: the crafted canvas of tests/tonemap_cases.py. The two CPU statements of the resolve (oracle/srt_oracle.c orc_average in C,
tests/denoise_ref.py tonemap in numpy) agree on it byte for byte for every divisor; the reference build's bytes of its +-8 ulp
subset, stored in tests/golden/ref_checks.npz, are the oracle's; and the set tells the near-misses of the resolve apart -- a
condition on the inputs that tests/test_gpu_tonemap_edges.py feeds to the device, checked here and never against a kernel."""
import ctypes

import numpy as np
import pytest

import denoise_ref as D
import golden_io
import tonemap_cases as TC

F32 = np.float32


def divided(img, ticks):
    with np.errstate(all="ignore"):
        return (np.asarray(img, F32)[..., :3] / TC.f32_ticks(ticks)).astype(F32)


def test_set_is_what_it_says():
    """The windows sit where the byte changes, the layout shows every value to every channel, the alpha lane is garbage."""
    b = TC.boundaries()
    ks = np.arange(1, 256)
    assert np.all(TC.byte(b.view(F32)) >= ks) and np.all(TC.byte((b - 1).view(F32)) < ks)
    assert abs(float(b[254:255].view(F32)[0]) - 7.2416) < 1e-3
    assert TC.windows(TC.WIDE).shape == (255, 129) and TC.windows(TC.NARROW).shape == (255, 17)
    assert TC.f32_ticks(16777217) == F32(2.0 ** 24) and TC.f32_ticks(4294967295) == F32(2.0 ** 32)
    img = TC.natural_image()
    assert img.shape[1] == TC.WIDTH and img.shape[0] * img.shape[1] == len(TC.values())
    flat = img.reshape(-1, 4)
    want = np.sort(TC.values().view(np.uint32))
    for ch in range(3):
        assert np.array_equal(np.sort(flat[:, ch].copy().view(np.uint32)), want), ch
    assert not np.isfinite(flat[0::2, 3]).any() and np.all(flat[1::2, 3] == F32(1e30))
    for count in (1, 255, 257):
        assert TC.pixels(count).shape == (count, 4)
    # after the division the divided windows are on the boundaries again: most of a window's values come back exactly
    for t in TC.DIVIDED_TICKS:
        back = (TC.divided_windows(t) / TC.f32_ticks(t)).astype(F32)
        assert TC.near_boundary(back, TC.NARROW + 1) == back.size, t
    # the edges the issue names, with the bytes the rule gives them (x * x * 2.51 overflows from about 1.2e19: inf / inf, byte 0)
    e = {float(x): int(k) for x, k in zip(TC.edges(), TC.byte(TC.edges())) if x == x}
    assert e[float(F32(1e19))] == 255 and e[float(F32(1.18e19))] == 255 and e[float(F32(1.2e19))] == 0
    assert e[float(F32(-1e19))] == 255 and e[float(np.inf)] == 0 and e[float(-np.inf)] == 0 and e[float(np.finfo(F32).max)] == 0
    assert np.all(TC.byte(TC.edges()[np.isnan(TC.edges())]) == 0)
    assert 0 < float(D._aces1(F32(-0.012))) < 1e-3  # x * 2.51 + 0.03 changes sign just above: a tiny positive fit, byte 0


@pytest.mark.parametrize("ticks", TC.TICKS)
def test_c_and_numpy_statements_agree(oracle, ticks):
    """oracle.average(ticks, set) == denoise_ref.tonemap(set / ticks), byte for byte; ticks = 0 divides by zero (+-inf, and NaN
    for +-0 / 0 and NaN / 0: every colour byte 0), 16777217 and 4294967295 convert to 2^24 and 2^32."""
    img = TC.natural_image()
    got = oracle.average(ticks, img)
    assert np.array_equal(got, D.tonemap(divided(img, ticks))), ticks
    assert np.all(got[..., 0] == 255)  # the alpha byte, whatever the canvas's alpha lane holds
    if ticks == 0:
        assert not got[..., 1:].any()


def test_reference_build_agrees_on_the_narrow_subset(oracle, ref):
    """The reference's own `average` (render.cl compiled for x86-64) on the +-8 ulp windows, the divided windows and the edges:
    its stored bytes (tests/golden/ref_checks.npz "tonemap/<ticks>", make_golden.py --ref-checks) are the oracle's, and so are
    the live build's where oracle/_ref is built. "tonemap/disagree" lists inputs on which the two differed when the fixture was
    made: none."""
    stored = golden_io.load_ref_checks()
    img = TC.image(TC.narrow_values())
    assert stored["tonemap/disagree"].size == 0
    for ticks in TC.TICKS:
        got = oracle.average(ticks, img)
        assert np.array_equal(got, stored[f"tonemap/{ticks}"]), ticks
        if ref is not None:
            assert np.array_equal(got, ref.average(ticks, img)), ticks


@pytest.mark.parametrize("spp", [1, 4, 12])
def test_zero_scene_renders_exactly_zero(oracle, sky, spp):
    """tonemap_cases.zero_scene() at the size and the sample counts tests/test_gpu_tonemap_edges.py renders it with: every
    channel of the oracle's canvas is +0 bit for bit, so adding the frame to a canvas changes nothing but -0."""
    from simple_raytracer_amd import records as R, scenes as S
    shapes, tris, mats = TC.zero_scene()
    h, w = TC.natural_image().shape[:2]
    rd = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=777)
    canvas = oracle.render(rd, R.scene_data(len(shapes)), shapes, tris, mats, sky)
    assert not canvas.view(np.uint32).any()


# ---- near-misses of the rule, restated in float32 steps ----------------------------------------------------------------------

_fmaf = ctypes.CDLL("libm.so.6").fmaf
_fmaf.restype = ctypes.c_float
_fmaf.argtypes = [ctypes.c_float] * 3
_fma = np.frompyfunc(lambda a, b, c: _fmaf(a, b, c), 3, 1)


def fma(a, b, c):
    """IEEE fusedMultiplyAdd in float32, element by element (libm's fmaf)."""
    return _fma(np.asarray(a, F32), F32(b), F32(c)).astype(F32)


def aces_raw(x, contracted=False):
    a, b, c, d, e = F32(2.51), F32(0.03), F32(2.43), F32(0.59), F32(0.14)
    with np.errstate(all="ignore"):
        p, q = (fma(x, a, b), fma(x, c, d)) if contracted else (x * a + b, x * c + d)
        return ((x * p) / (x * q + e)).astype(F32)


def clamp01(v, nan_dropping=False):
    with np.errstate(all="ignore"):
        if nan_dropping:
            return np.fmin(np.fmax(v, F32(0)), F32(1)).astype(F32)
        v = np.where(v < F32(0), F32(0), v)
        return np.where(F32(1) < v, F32(1), v).astype(F32)


def variant_bytes(canvas, ticks, contracted=False, reciprocal=False, sqrt_nudge=0, nearest=False, saturate=False):
    """The resolve's bytes of canvas values (any shape) with the named slips applied; with none, denoise_ref's bytes."""
    n = TC.f32_ticks(ticks)
    with np.errstate(all="ignore"):
        x = (canvas * (F32(1) / n) if reciprocal else canvas / n).astype(F32)
        s = np.sqrt(clamp01(aces_raw(x, contracted)))
        if sqrt_nudge:
            s = np.where(s > 0, np.nextafter(s, F32(np.inf if sqrt_nudge > 0 else -np.inf)), s).astype(F32)
        v = s * F32(255.0)
        ok = v == v
        i = (np.rint(np.where(ok, v, 0)) if nearest else np.trunc(np.where(ok, v, 0))).astype(np.int64)
        i = np.minimum(i, 255) if saturate else i & 255
        return np.where(ok, i, 0).astype(np.uint8)


def test_set_tells_near_misses_apart():
    """Bytes of the crafted list (54649 values, one channel) on which a slip differs from the rule, summed over the divisors
    1, 3, 7 and 10 (4 x 54649 bytes) unless said otherwise:

      (a) x * a + b and x * c + d of the fit contracted to fma           632  (193 / 144 / 140 / 155 at n = 1 / 3 / 7 / 10)
      (b) c * (1 / n) for c / n (n = 3, 7, 10; n = 1 cannot differ)      426  (137 / 224 / 65 at n = 3 / 7 / 10)
      (c) sqrt one ulp up                                               2913
          sqrt one ulp down                                            39362  (most of them saturated values: 1.0 -> 254)
      (d) the byte rounded to nearest, not truncated                   90364
      (e) clamp by a NaN-dropping min / max: the BYTE cannot differ (NaN -> 0.0 -> byte 0, the byte of a NaN), so the fit's
          float is compared: 0.0 where the rule gives NaN, on 9 values of the list at n = 1 (the NaNs, +-inf, +-FLT_MAX and
          +-1.2e19, where the fit is inf / inf)
      (f) a saturating conversion for `& 255`: cannot be told apart on any input and is dropped. The clamp bounds the fit by 1,
          sqrt(1) * 255 = 255 exactly, and 255 & 255 = 255 = min(255, 255); nothing above 255 reaches the conversion.

    (a)-(d) must each move at least one byte, or the windows are too narrow. Applying one of them to a scratch copy of
    csrc/tonemap.h or csrc/frame.hip and running variant_bytes with the same switch shows which crafted inputs catch it."""
    v = TC.values()
    ticks = (1, 3, 7, 10)
    rule = {t: variant_bytes(v, t) for t in ticks}
    for t in ticks:
        assert np.array_equal(rule[t], TC.byte(divided(v[:, None], t)[:, 0])), t  # no switch: the reference itself

    def differing(**kw):
        return {t: int(np.sum(variant_bytes(v, t, **kw) != rule[t])) for t in ticks}

    counts = {
        "a": differing(contracted=True),
        "b": differing(reciprocal=True),
        "c_up": differing(sqrt_nudge=+1),
        "c_down": differing(sqrt_nudge=-1),
        "d": differing(nearest=True),
        "f": differing(saturate=True),
    }
    print({k: (sum(c.values()), c) for k, c in counts.items()})
    for k in ("a", "c_up", "c_down", "d"):
        assert sum(counts[k].values()) > 0, k
    assert counts["b"][1] == 0 and all(counts["b"][t] > 0 for t in (3, 7, 10)), counts["b"]
    assert sum(counts["f"].values()) == 0  # (f): not a property of the set, see above
    # (e): on the fit's float
    raw = aces_raw(v)
    kept, dropped = clamp01(raw), clamp01(raw, nan_dropping=True)
    assert np.array_equal(kept.view(np.uint32), D._aces1(v).view(np.uint32))
    nan = np.isnan(kept)
    print("e", int(nan.sum()))
    assert nan.sum() > 0 and np.all(dropped[nan] == 0) and np.array_equal(kept[~nan], dropped[~nan])
    assert not rule[1][nan].any()  # ... and the byte is 0 either way
