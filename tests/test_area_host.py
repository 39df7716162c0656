"""CPU: the host part of area selection (include/srt_abi.h "area selection"; csrc/area_host.h) -- srt_area_mask_host against the
numpy restatement of the definition (tests/area_ref.py) bit for bit on directed polygons and rectangles and on seeded random
polygons, srt_area_check_host at the edges of what it accepts, the records' sizes against the records.py mirror, and the same code
as a program of its own under sanitizers (tests/csrc/area_host_check.cpp). Everything is an integer: every comparison is ==."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import area_ref as AR
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
W, H = AR.W, AR.H
SEED, N_RANDOM = 12, 300


def both(rect, lasso, w=W, h=H):
    got = T.area_mask(rect, lasso, w, h)
    want = AR.mask(rect, lasso, w, h)
    assert got.shape == want.shape == (h, w) and got.dtype == bool
    assert np.array_equal(got, want), (rect, lasso, np.argwhere(got != want)[:5])
    return want


@pytest.mark.parametrize("name", sorted(AR.LASSOS))
def test_directed_lassos_equal_the_restatement(name):
    lasso = AR.LASSOS[name]
    m = both((0, 0, W, H), lasso)
    assert m.any() != (name in AR.EMPTY), name
    assert not m.all()
    sub = both(AR.RECTS["inside"], lasso)  # intersected with a smaller rectangle
    assert np.array_equal(sub, m & AR.mask(AR.RECTS["inside"], None, W, H))
    near = lambda c, d: c - d if abs(c) < AR.COORD_MAX // 2 else c  # (the far vertices stay where they are)
    one = both((0, 0, 1, 1), [(near(x, 30), near(y, 15)) for x, y in lasso], 1, 1)  # the 1 x 1 frame, the polygon moved over it
    assert one.shape == (1, 1)


def test_orientation_does_not_matter():
    for name in ("convex", "bow_tie"):
        a, b = both((0, 0, W, H), AR.LASSOS[name]), both((0, 0, W, H), AR.LASSOS[name + "_reversed"])
        assert np.array_equal(a, b) and 0.05 < a.mean() < 0.95, name
    rolled = AR.LASSOS["concave_U"][3:] + AR.LASSOS["concave_U"][:3]  # another first vertex
    assert np.array_equal(both((0, 0, W, H), rolled), both((0, 0, W, H), AR.LASSOS["concave_U"]))


def test_centres_on_an_edge_do_not_count_for_it():
    """the 45-degree edge from corner (3, 3) to (33, 33) passes through the centres of pixels (k, k): with the region below it
    inside, those pixels are outside -- for either direction of the polygon"""
    for lasso in (AR.LASSOS["diagonal_through_centres"], AR.LASSOS["diagonal_through_centres"][::-1]):
        m = both((0, 0, W, H), lasso)
        for k in range(3, 33):
            assert not m[k, k], k
        for k in range(4, 33):
            assert m[k, k - 1] and not m[k - 1, k], k  # the pixel under the diagonal is inside, the one above is not
    m = both((0, 0, W, H), AR.LASSOS["half_pixel_diagonal"])
    assert 0.05 < m.mean() < 0.95


def test_far_vertices_need_the_int64_range():
    m = both((0, 0, W, H), AR.LASSOS["far_sliver"])
    # a band of whole rows between two nearly level edges two million pixels long: the upper one passes 2^-21 of a pixel under
    # row 5's centres, the lower one as much over row 30's
    assert m[6:30].all() and not m[:6].any() and not m[30:].any()
    m = both((0, 0, W, H), AR.LASSOS["far_outside"])
    assert 0.05 < m.mean() < 0.95
    # a product of two 2^22 differences is 2^44: computed in int32 it would wrap to 0 and the mask would be empty or full


def test_zigzag_has_all_256_vertices():
    lasso = AR.LASSOS["zigzag_256"]
    assert len(lasso) == AR.MAX_VERTICES == R.AREA_MAX_VERTICES
    m = both((0, 0, W, H), lasso)
    assert 0.05 < m.mean() < 0.95 and m[30].all() and not m[2].any() and 10 < m[10].sum() < 60


@pytest.mark.parametrize("name", sorted(AR.RECTS))
def test_rectangles_are_clipped_to_the_frame(name):
    rect = AR.RECTS[name]
    m = both(rect, None)
    x0, y0, x1, y1 = rect
    want = max(0, min(x1, W) - max(x0, 0)) * max(0, min(y1, H) - max(y0, 0))
    assert m.sum() == want
    if name.startswith(("outside", "empty")):
        assert want == 0
    both(rect, AR.LASSOS["bow_tie"])
    both(rect, None, 1, 1)
    both(rect, None, 3, 2)


def random_polygon(rng):
    """a star (sorted angles) two times in three, else vertices in any order (self-intersecting), around a point of the frame"""
    n = int(rng.integers(3, 41))
    cx, cy = rng.uniform(20, 50), rng.uniform(10, 27)
    ang = rng.uniform(0, 2 * np.pi, n)
    if rng.integers(0, 3) < 2:
        ang = np.sort(ang)
        rad = rng.uniform(0.55, 1.3, n)
    else:
        rad = rng.uniform(0.9, 1.6, n)
    return [(int(round(cx + 40 * r * np.cos(a))), int(round(cy + 22 * r * np.sin(a)))) for a, r in zip(ang, rad)]


def test_random_polygons_equal_the_restatement():
    rng = np.random.default_rng(SEED)
    for k in range(N_RANDOM):
        lasso = random_polygon(rng)
        m = both((0, 0, W, H), lasso)
        assert 0.05 <= m.mean() <= 0.95, (k, m.mean())  # none passes on an empty or a full mask


def test_check_refuses_what_the_interface_says():
    tri = [(0, 0), (5, 0), (0, 5)]
    M = AR.COORD_MAX
    assert T.area_check_host((0, 0, 4, 4)) and T.area_check_host((3, 3, 3, 3)) and T.area_check_host((-5, -9, 100000, 2 ** 31 - 1))
    assert T.area_check_host((0, 0, 4, 4), tri) and T.area_check_host((0, 0, 4, 4), AR.zigzag(256))
    assert T.area_check_host((0, 0, 4, 4), [(M, -M), (-M, M), (M, M)])
    assert not T.area_check_host((0, 0, 4, 4), AR.zigzag(256) + [(1, 1)])  # 257
    for n in (1, 2):
        assert not T.area_check_host((0, 0, 4, 4), tri[:n]), n
    for k in range(3):
        for axis in range(2):
            for bad in (M + 1, -M - 1, 2 ** 31 - 1, -2 ** 31):
                v = [list(p) for p in tri]
                v[k][axis] = bad
                assert not T.area_check_host((0, 0, 4, 4), v), (k, axis, bad)
    assert not T.area_check_host((0, 0, 4, 4), None, n_vertices=3)  # vertices NULL with a count
    assert not T.area_check_host((0, 0, 4, 4), None, flags=1)
    assert not T.area_check_host((0, 0, 4, 4), None, reserved=[1, 0]) and not T.area_check_host((0, 0, 4, 4), None, reserved=[0, 1])
    assert not T.area_check_host((5, 0, 4, 4)) and not T.area_check_host((0, 5, 4, 4))
    lib = T.load_library()
    assert lib.srt_area_check_host(None, None) != 0
    a, _ = T.area_record((0, 0, 4, 4))
    mask = np.full(12, 0xEE, np.uint8)
    assert lib.srt_area_mask_host(T._ptr(a), None, 4, 3, T._ptr(mask), 11) != 0 and (mask == 0xEE).all()  # one byte short
    assert lib.srt_area_mask_host(T._ptr(a), None, 4, 3, None, 12) != 0 and lib.srt_area_mask_host(T._ptr(a), None, 0, 3, T._ptr(mask), 12) != 0
    assert lib.srt_area_mask_host(T._ptr(a), None, 4, 3, T._ptr(mask), 12) == 0 and set(mask.tolist()) == {1}


def test_records_and_header():
    sizes = (C.c_size_t * 2)()
    assert T.load_library().srt_area_sizes(sizes) == 0 and T.load_library().srt_area_sizes(None) != 0
    assert (sizes[0], sizes[1]) == (R.AREA.itemsize, R.AREA_SUMMARY.itemsize) == (32, 32)
    types = (ROOT / "include" / "srt_types.h").read_text()
    for name, value in (("SRT_AREA_MAX_VERTICES", R.AREA_MAX_VERTICES), ("SRT_AREA_AGG_ROUNDS", R.AREA_AGG_ROUNDS), ("SRT_SELECT_REPLACE", R.SELECT_REPLACE),
                        ("SRT_SELECT_ADD", R.SELECT_ADD), ("SRT_SELECT_SUBTRACT", R.SELECT_SUBTRACT), ("SRT_SELECT_TOGGLE", R.SELECT_TOGGLE)):
        assert re.search(rf"#define {name} {value}u?\b", types), name
    assert (AR.REPLACE, AR.ADD, AR.SUBTRACT, AR.TOGGLE) == (R.SELECT_REPLACE, R.SELECT_ADD, R.SELECT_SUBTRACT, R.SELECT_TOGGLE)
    body = re.search(r"typedef struct srt_area_summary \{(.*?)\} srt_area_summary;", types, re.S).group(1)
    assert re.findall(r"^\s*uint32_t (\w+)", body, re.M) == list(R.AREA_SUMMARY.names)
    for cls in (T.Tracer, T.TracerGroup):
        for name in ("area_coverage", "area_triangle_coverage", "select_area", "read_selection", "area_mask"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(T.Tracer.area_coverage_device)


def test_restated_counts_and_modes_on_a_known_plane():
    shape = np.full((4, 6), AR.NONE, np.uint32)
    shape[1:3, 1:4] = 2
    shape[3, :] = 0
    tri = np.full((4, 6), AR.NONE, np.uint32)
    tri[1:3, 1:4] = [[5, 5, 1], [1, 1, 1]]
    counts, s = AR.coverage(shape, (0, 0, 6, 4), None, 3)
    assert counts.tolist() == [6, 0, 6] and s == dict(area_pixels=24, hit_pixels=12, miss_pixels=12, distinct=2, target_pixels=0)
    counts, s = AR.coverage(shape, (2, 1, 9, 3), None, 2)  # shape 2 is beyond the array: dropped from counts, still a hit
    assert counts.tolist() == [0, 0] and s == dict(area_pixels=8, hit_pixels=4, miss_pixels=4, distinct=0, target_pixels=0)
    counts, s = AR.triangle_coverage(shape, tri, 2, 6, (0, 0, 6, 4), None)
    assert counts.tolist() == [0, 4, 0, 0, 0, 2] and s["target_pixels"] == 6 and s["distinct"] == 2 and s["hit_pixels"] == 12
    c = np.array([6, 0, 3, 1], np.uint32)
    assert AR.combine([1, 2], c, AR.REPLACE, 1).tolist() == [0, 2, 3] and AR.combine([1, 2], c, AR.ADD, 0).tolist() == [0, 1, 2, 3]
    assert AR.combine([1, 2], c, AR.SUBTRACT, 1).tolist() == [1] and AR.combine([1, 2], c, AR.TOGGLE, 3).tolist() == [0, 1]
    assert AR.segments((3, 2, 68, 4), 70, 37) == [(2, 3, 67), (2, 67, 68), (3, 3, 67), (3, 67, 68)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stand_alone_check_under_sanitizers(tmp_path):
    """tests/csrc/area_host_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program of its own: no report,
    exit status 0, and the masks it prints (made by g++'s build of area_host.h) equal the restatement's."""
    csrc = ROOT / "simple-raytracer_amd" / "csrc"
    exe, cases_file = tmp_path / "area_host_check", tmp_path / "cases.txt"
    cases = [(W, H, (0, 0, W, H), AR.LASSOS[n]) for n in sorted(AR.LASSOS)] + [(W, H, AR.RECTS["inside"], AR.LASSOS[n]) for n in sorted(AR.LASSOS)]
    cases += [(w, h, AR.RECTS[n], None) for n in sorted(AR.RECTS) for (w, h) in ((W, H), (1, 1), (3, 2))]
    cases += [(1, 1, (0, 0, 1, 1), AR.LASSOS["far_outside"]), (W, H, (0, 0, W, H), AR.LASSOS["convex"][:2])]  # the last one is refused
    cases_file.write_text("".join(f"{w} {h} {r[0]} {r[1]} {r[2]} {r[3]} {len(l or [])} " + " ".join(f"{x} {y}" for x, y in (l or [])) + "\n" for w, h, r, l in cases))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           f"-I{csrc}", str(ROOT / "tests/csrc/area_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(cases_file)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-400:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == len(cases) + 1
    for (w, h, rect, lasso), line in zip(cases[:-1], lines):
        want = "".join("1" if v else "0" for v in AR.mask(rect, lasso, w, h).reshape(-1))
        assert line == want, (w, h, rect, lasso)
    assert lines[len(cases) - 1] == "refused"
