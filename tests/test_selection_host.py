"""CPU: the host part of the selection overlay (include/srt_abi.h "selection overlay and the ID pass"; csrc/selection_host.h) --
the outline's alpha table against the numpy restatement (tests/selection_ref.py), the parameter check, the defaults, the
struct's size against the records.py mirror, and the same code as a program of its own under sanitizers
(tests/csrc/selection_host_check.cpp). The restatement itself is checked against brute force on small masks."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import selection_ref as SR
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
WIDTHS, ALPHAS = (1.0, 1.5, 2.75, 8.0), (0, 1, 128, 255)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_alpha_table_equals_the_restatement(width, alpha):
    got, radius = T.selection_alpha_table_host(width=width, outline=(alpha, 10, 20, 30))
    want, want_radius = SR.table(width, alpha)
    assert radius == want_radius and 1 <= radius <= R.SELECTION_MAX_WIDTH
    assert got.dtype == np.uint8 and len(got) == 2 * radius * radius + 1 <= R.SELECTION_TABLE_MAX
    assert np.array_equal(got, want), (width, alpha)
    assert got[0] == alpha  # d2 = 0 is fully covered


def test_alpha_table_refuses_a_short_array_and_bad_parameters():
    lib = T.load_library()
    p = T.selection_defaults()
    p["outline_width"] = 8.0
    table, radius = np.full(R.SELECTION_TABLE_MAX, 0xEE, np.uint8), C.c_int(-1)
    assert lib.srt_selection_alpha_table_host(T._ptr(p), T._ptr(table), 128, C.byref(radius)) != 0 and (table == 0xEE).all()
    assert lib.srt_selection_alpha_table_host(T._ptr(p), T._ptr(table), 129, C.byref(radius)) == 0 and radius.value == 8
    assert lib.srt_selection_alpha_table_host(T._ptr(p), T._ptr(table), 129, None) == 0
    assert lib.srt_selection_alpha_table_host(None, T._ptr(table), 129, None) != 0
    assert lib.srt_selection_alpha_table_host(T._ptr(p), None, 129, None) != 0
    p["outline_width"] = 0.5
    assert lib.srt_selection_alpha_table_host(T._ptr(p), T._ptr(table), 129, None) != 0


def test_check_refuses_what_the_interface_says():
    assert T.selection_check_host()
    for width in (1.0, 8.0, 2.75):
        assert T.selection_check_host(width=width)
    for width in (0.99, 8.01, float("nan"), float("inf"), -float("inf"), 0.0, -2.0):
        assert not T.selection_check_host(width=width), width
    for k in range(4):
        reserved = [0, 0, 0, 0]
        reserved[k] = 1
        assert not T.selection_check_host(reserved=reserved), k
    assert T.selection_check_host(enabled=0)
    for enabled in (2, -1, 1 << 20):
        assert not T.selection_check_host(enabled=enabled), enabled
    assert T.load_library().srt_selection_check_host(None) != 0


def test_defaults_pass_their_own_check():
    d = T.selection_defaults()
    assert T.load_library().srt_selection_check_host(T._ptr(d)) == 0
    assert d["enabled"] == 1 and d["outline_width"] == 2.0 and (d["reserved"] == 0).all()
    assert d["outline_argb"][0] == 255 and d["fill_argb"][0] == 0  # an opaque outline, no fill
    assert T.load_library().srt_selection_defaults(None) != 0


def test_struct_size_equals_the_mirror():
    sizes = (C.c_size_t * 1)()
    assert T.load_library().srt_selection_sizes(sizes) == 0
    assert sizes[0] == R.SELECTION_PARAMS.itemsize == 32
    assert [R.SELECTION_PARAMS.fields[n][1] for n in R.SELECTION_PARAMS.names] == [0, 4, 8, 12, 16]


def _brute(m, radius):
    h, w = m.shape
    out = np.full((h, w), SR.NONE, np.int64)
    for y in range(h):
        for x in range(w):
            for qy in range(max(0, y - radius), min(h, y + radius + 1)):
                for qx in range(max(0, x - radius), min(w, x + radius + 1)):
                    if m[qy, qx]:
                        out[y, x] = min(out[y, x], (qx - x) ** 2 + (qy - y) ** 2)
    return out


@pytest.mark.parametrize("shape,radius", [((1, 1), 8), ((2, 3), 8), ((9, 13), 1), ((9, 13), 3), ((20, 11), 8)])
def test_restated_distance_equals_brute_force(shape, radius):
    rng = np.random.default_rng(shape[0] * 100 + radius)
    for density in (0.0, 0.03, 0.5, 1.0):
        m = rng.random(shape) < density
        assert np.array_equal(SR.distance2(m, radius), _brute(m, radius)), (shape, radius, density)


def test_restated_composite_on_known_bytes():
    argb = np.array([[[255, 0, 100, 255], [255, 10, 20, 30], [255, 200, 200, 200]]], np.uint8)
    a = np.array([[255, 0, 128]], np.uint8)
    outline = np.array([[True, False, False]])
    out = SR.composite(argb, a, outline, (255, 1, 2, 3), (128, 50, 60, 70))
    assert out[0, 0].tolist() == [255, 1, 2, 3]  # a = 255: the colour itself
    assert out[0, 1].tolist() == [255, 10, 20, 30]  # a = 0: untouched
    assert out[0, 2].tolist() == [255, (200 * 127 + 50 * 128 + 127) // 255, (200 * 127 + 60 * 128 + 127) // 255, (200 * 127 + 70 * 128 + 127) // 255]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stand_alone_check_under_sanitizers(tmp_path):
    """tests/csrc/selection_host_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program of its own: no
    report, exit status 0, and the tables it prints (made by g++'s build of selection_host.h) equal the restatement's."""
    csrc = ROOT / "simple-raytracer_amd" / "csrc"
    exe = tmp_path / "selection_host_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", f"-I{csrc}", str(ROOT / "tests/csrc/selection_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == len(WIDTHS) * len(ALPHAS) + 1
    for line in lines[:-1]:
        f = line.split()
        width, alpha, radius, got = float.fromhex(f[0]), int(f[1]), int(f[2]), [int(v) for v in f[3:]]
        want, want_radius = SR.table(width, alpha)
        assert radius == want_radius and got == want.tolist(), line
