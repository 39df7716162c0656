"""Noise metering without a GPU: the ABI's host-only entry points (defaults, validation, the percentile and the stopping rule)
and the properties of the numpy restatement (tests/noise_ref.py) the GPU tests compare the device with."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_ref as N

F32 = np.float32


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


SYMBOLS = ["srt_noise_defaults", "srt_noise_check_host", "srt_noise_evaluate_host", "srt_set_noise_meter", "srt_meter_noise", "srt_poll_noise",
           "srt_read_noise", "srt_resolve_noise_view", "srt_render_until", "srt_last_meter_ran", "srt_selftest_noise_meter",
           "srt_group_set_noise_meter", "srt_group_meter_noise", "srt_group_poll_noise", "srt_group_read_noise", "srt_group_resolve_noise_view",
           "srt_group_read_noise_view"]


def test_symbols_exist(T):
    lib = T.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in T.ABI_SYMBOLS, s


def test_defaults(T):
    d = T.noise_defaults()
    assert d["enable"] == 1 and d["permille"] == 950 and d["min_samples"] == 16 and d["check_every"] == 4 and d["reserved"] == [0, 0]
    assert F32(d["threshold"]) == F32(0.05) and F32(d["luminance_floor"]) == F32(0.01)
    assert {k: d[k] for k in ("permille", "min_samples", "check_every")} == {k: N.DEFAULTS[k] for k in ("permille", "min_samples", "check_every")}
    assert C.sizeof(T.NoiseParams) == 32 and C.sizeof(T.NoiseResult) == 32
    assert T.noise_check_host()


def up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def down(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


@pytest.mark.parametrize("field,good,bad", [
    ("threshold", [2.0 ** -24, 2.0 ** 8, 0.05], [down(2.0 ** -24), up(2.0 ** 8), 0.0, -1.0, float("nan"), float("inf")]),
    ("luminance_floor", [2.0 ** -20, 2.0 ** 20, 0.01], [down(2.0 ** -20), up(2.0 ** 20), 0.0, float("nan"), float("inf"), -0.01]),
    ("permille", [1, 1000], [0, 1001, -1]),
    ("min_samples", [1, 2 ** 32 - 1], [0]),
    ("check_every", [1, 65536], [0, 65537, -4]),
    ("reserved", [[0, 0]], [[1, 0], [0, 1]]),
])
def test_check_host_rejects_each_field_at_its_first_invalid_value(T, field, good, bad):
    for v in good:
        assert T.noise_check_host(**{field: v}), (field, v)
    for v in bad:
        assert not T.noise_check_host(**{field: v}), (field, v)


def test_eighths_table_is_two_to_the_k_eighths():
    assert len(N.EIGHTHS) == 8
    for k in range(8):
        # 2^(k/8) from an integer eighth root in exact arithmetic, rounded to float once: the float32 whose 8th power brackets 2^k
        e = N.EIGHTHS[k]
        lo, hi = np.nextafter(e, F32(0)), np.nextafter(e, F32(4))
        exact = lambda f: int(np.float64(f) * 2 ** 24)  # noqa: E731 (an integer, exactly: f has 24 significant bits and lies in [1, 2))
        half_lo, half_hi = exact(lo) + exact(e), exact(e) + exact(hi)  # twice the rounding boundaries, scaled by 2^24
        assert half_lo ** 8 <= (2 ** k) * (2 ** 25) ** 8 <= half_hi ** 8, k
        assert e == F32(2.0 ** (k / 8.0))


def test_level_is_monotone_in_the_bin_and_matches_the_library(T):
    levels = [N.level_of(b) for b in range(256)]
    assert all(a < b for a, b in zip(levels, levels[1:]))
    assert levels[7] == F32(2.0 ** -23) and levels[255] == F32(2.0 ** 8) and levels[0] == F32(N.EIGHTHS[1] * F32(2.0 ** -24))
    for b in range(256):
        hist = np.zeros(256, np.uint32)
        hist[b] = 5
        got = T.noise_evaluate_host(hist, (5, 0, 0), 3, 64)
        assert got["level_bin"] == b and F32(got["level"]).view(np.uint32) == levels[b].view(np.uint32), b
        # The bins cut an octave by mantissa bits, at 1 + k / 8; the level quotes 2^(k / 8). At an octave's end the two agree: the
        # level is the smallest float of the next bin. Inside, the level lies below the bin's own upper edge, in the bin itself.
        if b < 255 and (b + 1) % 8 == 0:
            assert int(N.bin_of(levels[b])) == b + 1 and int(N.bin_of(np.nextafter(levels[b], F32(0)))) == b
        elif b < 255:
            assert int(N.bin_of(levels[b])) == b


def test_r_doubles_bin_moves_by_eight():
    rng = np.random.default_rng(5)
    r = np.exp2(rng.uniform(-23, 6, 500)).astype(F32)
    assert np.array_equal(N.bin_of(r * F32(2)), N.bin_of(r) + 8)
    assert int(N.bin_of(F32(0))) == 0 and int(N.bin_of(F32(1e-40))) == 0 and int(N.bin_of(F32(2.0 ** -24))) == 0
    assert int(N.bin_of(down(2.0 ** 8))) == 255 and int(N.bin_of(F32(3e38))) == 255 and int(N.bin_of(F32(2.0 ** -24 * 1.125))) == 1 and int(N.bin_of(down(2.0 ** -24 * 1.125))) == 0


def noise_frame(n, seed=11):
    rng = np.random.default_rng(seed)
    canvas = np.zeros((n, 4), F32)
    canvas[:, :3] = rng.uniform(0.0, 3.0, (n, 3))
    L = N.D.lum(canvas[:, :3])
    moments = (L * L * (1 + np.exp2(rng.uniform(-12, 4, n)))).astype(F32)
    return canvas, moments


def test_below_is_monotone_in_the_threshold():
    canvas, moments = noise_frame(4000)
    last = -1
    for k in range(-24, 9):
        got = N.meter(canvas, moments, 1, 4, threshold=2.0 ** k)
        assert got["below"] >= last and got["metered"] == 4000 and got["left_out"] == 0
        last = got["below"]
    assert last == 4000 and N.meter(canvas, moments, 1, 4, threshold=2.0 ** -24)["below"] < 4000


def test_negative_variance_from_rounding_is_bin_zero_not_left_out():
    # a constant pixel: m2 = L * L in exact arithmetic; where the division by T rounds m2 below L * L the difference is negative
    T_, P = 3, 6
    vals = np.linspace(0.3, 2.9, 257).astype(F32)
    canvas = np.zeros((len(vals), 4), F32)
    canvas[:, :3] = (vals * F32(T_))[:, None]
    L = N.D.lum((canvas[:, :3] / F32(T_)).astype(F32))
    moments = (L * L * F32(T_)).astype(F32)
    with np.errstate(all="ignore"):
        v = (moments / F32(T_)).astype(F32) - (L * L).astype(F32)
    assert (v < 0).any()  # the case exists in this frame
    got = N.meter(canvas, moments, T_, P)
    assert got["left_out"] == 0 and got["metered"] == len(vals)
    assert got["hist"][0] == int(np.sum(v <= 0)) and (got["bins"][v < 0] == 0).all()


def test_stopping_rule_and_percentile_against_the_library(T):
    rng = np.random.default_rng(3)
    for trial in range(50):
        hist = np.zeros(256, np.uint32)
        for b in rng.integers(0, 256, rng.integers(1, 6)):
            hist[b] += rng.integers(1, 2000)
        metered = int(hist.sum())
        below = int(rng.integers(0, metered + 1))
        permille, min_samples, P = int(rng.integers(1, 1001)), int(rng.integers(1, 40)), int(rng.integers(1, 40))
        want = N.evaluate(hist, metered, below, P, permille, min_samples)
        got = T.noise_evaluate_host(hist, (metered, 7, below), 5, P, permille=permille, min_samples=min_samples)
        assert (got["level_bin"], got["converged"]) == (want[0], want[2]), trial
        assert F32(got["level"]).view(np.uint32) == want[1].view(np.uint32)
        assert (got["metered"], got["left_out"], got["below"], got["dispatches"], got["samples"]) == (metered, 7, below, 5, P)
    # the exact integer boundary, and min_samples over everything
    hist = np.zeros(256, np.uint32)
    hist[40] = 1000
    assert T.noise_evaluate_host(hist, (1000, 0, 949), 4, 16)["converged"] == 0
    assert T.noise_evaluate_host(hist, (1000, 0, 950), 4, 16)["converged"] == 1
    assert T.noise_evaluate_host(hist, (1000, 0, 1000), 4, 15)["converged"] == 0
    empty = T.noise_evaluate_host(np.zeros(256, np.uint32), (0, 12, 0), 4, 16)
    assert (empty["converged"], empty["level_bin"], float(empty["level"])) == (0, -1, 0.0)
    # the percentile: the bin in which the ascending count first reaches ceil(metered * permille / 1000)
    hist = np.zeros(256, np.uint32)
    hist[10], hist[200] = 950, 50
    assert T.noise_evaluate_host(hist, (1000, 0, 0), 4, 16)["level_bin"] == 10
    hist[10], hist[200] = 949, 51
    assert T.noise_evaluate_host(hist, (1000, 0, 0), 4, 16)["level_bin"] == 200
    assert math.isclose(float(N.level_of(200)), 2.0 ** (201 / 8 - 24), rel_tol=1e-6)
