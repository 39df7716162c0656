"""CPU: bloom for the resolve (include/srt_abi.h srt_set_bloom). The entry points are exported and declared, the host-only
validation accepts the defaults and rejects each field at its first invalid value, and the numpy restatement the GPU tests compare
with (tests/bloom_ref.py) has the properties the filters' weights and the prefilter's curve are chosen for."""
import re
from pathlib import Path

import numpy as np
import pytest

import bloom_ref as B

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def test_entry_points_are_declared_and_exported(T):
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include/srt_abi.h").read_text(), flags=re.S)
    lib = T.load_library()
    for name in ("srt_bloom_defaults", "srt_bloom_check_host", "srt_set_bloom", "srt_group_set_bloom", "srt_read_bloom",
                 "srt_group_read_bloom", "srt_last_resolve_bloomed", "srt_group_last_resolve_bloomed"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in T.ABI_SYMBOLS and hasattr(lib, name), name


def test_defaults_are_the_documented_ones_and_valid(T):
    d = T.bloom_defaults()
    assert (d["enable"], d["levels"], d["reserved"]) == (1, 6, 0)
    assert (d["threshold"], d["knee"], d["clamp"]) == (1.0, 0.5, 64.0) and d["intensity"] == F32(0.1) and d["scatter"] == F32(0.7)
    assert T.bloom_check_host()
    for k, v in B.DEFAULTS.items():
        assert F32(d[k]) == F32(v), k
    assert T.BLOOM_MAX_LEVELS == B.MAX_LEVELS == 8
    types = (ROOT / "include/srt_types.h").read_text()
    assert re.search(r"#define\s+SRT_BLOOM_MAX_LEVELS\s+8\b", types)


up = lambda v: float(np.nextafter(F32(v), F32(np.inf)))  # noqa: E731
down = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))  # noqa: E731
tiny = float(np.finfo(F32).smallest_subnormal)
ACCEPTED = [dict(threshold=0.0, knee=0.0), dict(threshold=3e38, knee=3e38), dict(knee=0.0), dict(knee=1.0), dict(intensity=0.0),
            dict(intensity=16.0), dict(scatter=0.0), dict(scatter=1.0), dict(clamp=0.0), dict(clamp=tiny), dict(clamp=3e38),
            dict(levels=1), dict(levels=8)]
REJECTED = [dict(threshold=-tiny, knee=0.0), dict(threshold=float("inf")), dict(threshold=float("nan")),
            dict(knee=-tiny), dict(knee=up(1.0)), dict(knee=float("nan")), dict(threshold=0.25),  # (the default knee 0.5 > 0.25)
            dict(intensity=-tiny), dict(intensity=up(16.0)), dict(intensity=float("inf")), dict(intensity=float("nan")),
            dict(scatter=-tiny), dict(scatter=up(1.0)), dict(scatter=float("nan")),
            dict(clamp=-tiny), dict(clamp=-1.0), dict(clamp=float("inf")), dict(clamp=float("nan")),
            dict(levels=0), dict(levels=-1), dict(levels=9), dict(reserved=1), dict(reserved=-1)]


@pytest.mark.parametrize("kw", ACCEPTED, ids=str)
def test_check_host_accepts_the_last_valid_values(T, kw):
    assert T.bloom_check_host(**kw)


@pytest.mark.parametrize("kw", REJECTED, ids=str)
def test_check_host_rejects_each_field_at_its_first_invalid_value(T, kw):
    assert not T.bloom_check_host(**kw)


def test_check_host_rejects_null(T):
    assert T.load_library().srt_bloom_check_host(None) != 0


@pytest.mark.parametrize("c", [2.0 ** -20, 1.0, 2.0 ** 9])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (7, 5), (16, 9)])
def test_a_power_of_two_image_is_a_fixed_point_of_reduce_and_expand(w, h, c):
    """(c + c) + 3 (c + c) = 8c, 0.75c + 0.25c = c: all exact, so the filters' weights sum to 1 to the bit, edges included."""
    img = np.full((h, w, 3), c, F32)
    r = B.reduce(img)
    assert r.shape == ((h + 1) // 2, (w + 1) // 2, 3) and np.array_equal(r.view(np.uint32), np.full_like(r, c).view(np.uint32))
    e = B.expand(r, w, h)
    assert np.array_equal(e.view(np.uint32), img.view(np.uint32))


def test_impulse_response_of_reduce_then_expand_is_mirror_symmetric():
    """On an even-sized image the taps 2i-1 .. 2i+2 and the expand phases map onto themselves under a flip, and a + d, b + c
    commute: the response to the flipped impulse is the flipped response, bit for bit."""
    w, h = 12, 8
    rng = np.random.RandomState(5)
    for x, y in [(0, 0), (w - 1, 0), (0, h - 1), (5, 3), (6, 4), (w - 2, h - 1), (3, 0)]:
        v = rng.uniform(0.5, 40.0, 3).astype(F32)
        a, b = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
        a[y, x], b[h - 1 - y, w - 1 - x] = v, v
        ra, rb = B.expand(B.reduce(a), w, h), B.expand(B.reduce(b), w, h)
        assert ra.any() and np.array_equal(ra.view(np.uint32), rb[::-1, ::-1].view(np.uint32)), (x, y)


def test_prefilter_curve():
    T_, K, Cl = F32(1.0), F32(0.5), F32(64.0)
    L = np.concatenate([np.linspace(1e-3, 3.0, 4001), np.exp2(np.linspace(-20, 12, 2001))]).astype(F32)
    L = np.unique(np.concatenate([L, [T_ - K, np.nextafter(T_ - K, F32(0)), np.nextafter(T_ - K, F32(2)), T_, T_ + K, np.nextafter(T_ + K, F32(4)),
                                      Cl + T_, F32(1000.0)]]).astype(F32))
    g = B.soft_threshold(L, T_, K, Cl)
    assert np.all(g[L <= T_ - K] <= 0)                       # 0 at and below threshold - knee (the pixel contributes nothing)
    assert np.all(g[L > T_ - K] > 0)
    above = L >= T_ + K
    assert np.array_equal(g[above & (L - T_ <= Cl)], (L - T_)[above & (L - T_ <= Cl)])  # L - threshold above the knee
    assert g.max() == Cl and np.all(g[L - T_ >= Cl] == Cl)   # never above clamp
    assert np.all(np.diff(g) >= 0)                           # monotone
    # continuous through the knee: at its two ends the quadratic meets 0 and L - threshold exactly, and no step between samples
    # 7.5e-4 apart exceeds the slope bound 1 by more than rounding
    assert B.soft_threshold(T_ - K, T_, K, Cl) == 0 and B.soft_threshold(T_ + K, T_, K, Cl) == K
    knee = (L >= T_ - K) & (L <= T_ + K)
    assert np.all(np.diff(g[knee]) <= np.diff(L[knee]) * F32(1.0001) + F32(1e-7))
    # knee 0: a hard threshold; clamp 0: no limit
    assert np.array_equal(B.soft_threshold(L, T_, 0.0, 0.0), L - T_)
    # the contribution: bright = x * (g / L) has luminance about g, is (0, 0, 0) below, and non-finite pixels contribute nothing
    x = np.array([[[2.0, 2.0, 2.0], [0.4, 0.4, 0.4], [np.nan, 1, 1], [np.inf, 1, 1], [-9.0, 1, 1], [0, 0, 0], [3e38, 3e38, 3e38], [1e-40, 5, 1]]], F32)
    b = B.prefilter(x, T_, K, Cl)
    assert np.all(b[0, 1:6] == 0) and not np.signbit(b[0, 1:6]).any()
    assert np.allclose(b[0, 6], Cl, rtol=1e-6)  # (the weights of lum sum to 1: 3e38 stays finite and is clamped)
    assert np.allclose(b[0, 0], 1.0, rtol=1e-6) and np.all(np.isfinite(b)) and b[0, 7, 1] > 0
    assert np.all(B.prefilter(np.full((1, 1, 3), 1e6, F32), T_, K, Cl) <= np.nextafter(Cl, F32(128)))


@pytest.mark.parametrize("w,h,sizes", [
    (1, 1, [(1, 1)]),
    (1, 9, [(1, 5), (1, 3), (1, 2), (1, 1)]),
    (131, 67, [(66, 34), (33, 17), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1)]),
    (1920, 1080, [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17), (15, 9), (8, 5)])])
def test_level_sizes_and_the_cut_off(w, h, sizes):
    assert B.level_sizes(w, h, 8) == sizes
    for n in range(1, 9):
        assert B.level_sizes(w, h, n) == sizes[:n]
    rng = np.random.RandomState(w)
    if w * h <= 131 * 67:
        x = np.exp2(rng.uniform(-2, 6, (h, w, 3))).astype(F32)
        ups = B.pyramid(x, B.params(levels=8))
        assert [(u.shape[1], u.shape[0]) for u in ups] == sizes
        assert B.bloomed_bytes(x, 1, 1.0, B.params(levels=8))[0].shape == (h, w, 4)
