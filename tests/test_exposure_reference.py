"""CPU: exposure for the resolve (include/srt_abi.h srt_set_exposure). The entry points are exported and declared, the host-only
validation accepts the defaults and rejects each field at its first invalid value, and the numpy restatement the GPU tests
compare with (tests/exposure_ref.py) has the bin rule of the header at the bin edges and at both ends of the range."""
import re
from pathlib import Path

import numpy as np
import pytest

import exposure_ref as E

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
    for name in ("srt_exposure_defaults", "srt_exposure_check_host", "srt_set_exposure", "srt_group_set_exposure", "srt_reset_exposure",
                 "srt_group_reset_exposure", "srt_read_exposure", "srt_group_read_exposure", "srt_last_resolve_exposed",
                 "srt_group_last_resolve_exposed"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in T.ABI_SYMBOLS and hasattr(lib, name), name


def test_defaults_are_the_documented_ones_and_valid(T):
    d = T.exposure_defaults()
    assert d["enable"] == 1 and d["mode"] == T.EXPOSURE_AUTO and d["ev"] == 0.0 and d["key"] == F32(0.18)
    assert (d["low_permille"], d["high_permille"], d["adapt"]) == (100, 950, 1.0)
    assert (d["min_ev"], d["max_ev"], d["reserved"]) == (-16.0, 16.0, [0, 0, 0])
    assert T.exposure_check_host()
    for k, v in E.DEFAULTS.items():
        assert F32(d[k]) == F32(v), k


above_32, below_1 = float(np.nextafter(F32(32), F32(64))), float(np.nextafter(F32(1), F32(0)))
ACCEPTED = [dict(ev=32.0), dict(ev=-32.0), dict(adapt=1.0), dict(adapt=below_1), dict(adapt=float(np.finfo(F32).smallest_subnormal)),
            dict(low_permille=0, high_permille=1), dict(low_permille=999, high_permille=1000), dict(low_permille=0, high_permille=1000),
            dict(key=float(np.finfo(F32).smallest_subnormal)), dict(min_ev=-32.0, max_ev=32.0), dict(min_ev=3.0, max_ev=3.0),
            dict(mode="manual"), dict(mode="auto")]
REJECTED = [dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=float(np.nextafter(F32(1), F32(2)))), dict(adapt=float("nan")),
            dict(low_permille=500, high_permille=500), dict(low_permille=500, high_permille=499), dict(low_permille=-1),
            dict(low_permille=1000, high_permille=1000), dict(high_permille=1001),
            dict(key=0.0), dict(key=-0.18), dict(key=float("inf")), dict(key=float("nan")),
            dict(ev=above_32), dict(ev=-above_32), dict(ev=float("inf")), dict(ev=float("nan")),
            dict(min_ev=-above_32), dict(max_ev=above_32), dict(min_ev=1.0, max_ev=float(np.nextafter(F32(1), F32(0)))),
            dict(min_ev=float("nan")), dict(max_ev=float("nan")), dict(min_ev=float("-inf")),
            dict(reserved=[1, 0, 0]), dict(reserved=[0, 1, 0]), dict(reserved=[0, 0, -1]), dict(mode=2), dict(mode=-1)]


@pytest.mark.parametrize("kw", ACCEPTED, ids=str)
def test_check_host_accepts_the_last_valid_values(T, kw):
    assert T.exposure_check_host(**kw)


@pytest.mark.parametrize("kw", REJECTED, ids=str)
def test_check_host_rejects_each_field_at_its_first_invalid_value(T, kw):
    assert not T.exposure_check_host(**kw)


def test_check_host_rejects_null(T):
    assert T.load_library().srt_exposure_check_host(None) != 0


def test_bin_rule_at_every_bin_edge():
    """Bin b starts at 2^(b / 4 - 32) taken down to two mantissa bits: 2^e * (1 + m / 4). The edge itself is in bin b, the
    largest float below it in bin b - 1, for every b = 1..255."""
    b = np.arange(1, E.BINS)
    edge = (np.ldexp(1.0, b // 4 - 32) * (1.0 + (b % 4) / 4.0)).astype(F32)
    below = np.nextafter(edge, F32(0))
    assert np.array_equal(E.bins_of(edge), b)
    assert np.array_equal(E.bins_of(below), b - 1)
    # a bin's centre in log2 is within a quarter octave of any value in it
    assert np.all(np.abs(np.log2(edge.astype(np.float64)) - ((b + 0.5) / 4.0 - 32.0)) <= 0.25)


def test_bin_rule_at_the_ends_and_what_is_left_out():
    fi = np.finfo(F32)
    assert E.bins_of(F32(2.0 ** -33)) == 0 and E.bins_of(F32(2.0 ** 33)) == 255
    assert E.bins_of(F32(2.0 ** -32)) == 0 and E.bins_of(np.nextafter(F32(2.0 ** 32), F32(0))) == 255 and E.bins_of(F32(2.0 ** 32)) == 255
    assert E.bins_of(F32(fi.smallest_subnormal)) == 0 and E.bins_of(F32(fi.tiny)) == 0 and E.bins_of(F32(fi.max)) == 255
    assert E.bins_of(F32(1.0)) == 128 and E.bins_of(F32(0.18)) == 4 * (32 - 3) + 1  # 0.18 = 2^-3 * 1.44
    left_out = np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], F32)
    assert np.all(E.bins_of(left_out) == -1)
    hist, counts = E.histogram(np.array([[1, 1, 1, 9], [0, 0, 0, 9], [np.nan, 1, 1, 9], [-4, 1, 1, 9]], F32), 1)
    assert counts == (1, 3) and hist[128] == 1 and hist.sum() == 1  # lum(1, 1, 1) = 1 to the bit; lum(-4, 1, 1) < 0; alpha never read


def test_trimmed_mean_window_and_adaptation_on_hand_computed_cases():
    hist = np.zeros(E.BINS, np.uint32)
    hist[100], hist[128], hist[200] = 10, 80, 10
    assert E.window(100, 100, 950) == (10, 95) and E.window(1, 100, 950) == (0, 1) and E.window(3, 999, 1000) == (2, 3)
    assert E.trimmed_mean(hist, 100, 900) == 128.5 / 4 - 32  # both tails cut away whole
    assert E.trimmed_mean(hist, 0, 1000) == (10 * (100.5 / 4 - 32) + 80 * (128.5 / 4 - 32) + 10 * (200.5 / 4 - 32)) / 100
    assert E.trimmed_mean(hist, 50, 100) == 100.5 / 4 - 32  # a window inside one bin
    assert E.trimmed_mean(np.zeros(E.BINS, np.uint32), 100, 950) is None
    m = E.Meter(adapt=0.5, key=1.0, low_permille=100, high_permille=900)
    l2, e = m.frame(hist)  # the first frame adopts its target
    assert l2 == F32(-(128.5 / 4 - 32)) and e == F32(2.0 ** -0.125)
    assert m.frame(np.zeros(E.BINS, np.uint32)) == (l2, e)  # nothing metered: unchanged
    hist2 = np.zeros(E.BINS, np.uint32)
    hist2[136] = 7  # two octaves brighter
    assert m.frame(hist2)[0] == F32(-0.125 - 1.0) and m.frame(hist2)[0] == F32(-0.125 - 1.5)
    m.reset()
    assert m.frame(hist2)[0] == F32(-2.125)
    assert E.Meter(key=1.0, max_ev=-3.0).frame(hist2)[0] == F32(-3.0) and E.Meter(key=1.0, min_ev=1.0, ev=0.5).frame(hist2)[0] == F32(1.5)
    assert E.manual(-3.0) == (F32(-3), F32(0.125)) and E.ulps(F32(1), np.nextafter(F32(1), F32(2))) == 1
