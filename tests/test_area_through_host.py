"""CPU: the host part of X-ray area selection (include/srt_abi.h "area selection, through"; csrc/area_through_host.h) -- the
library has the entry points and the ctypes signatures agree with the header, Python's through=False paths call the entry points
they always called, the tests' cameras see through (decided with the oracle alone), the reference counts as the definition says on
hand-made candidate lists, and the launch grid as a program of its own under sanitizers (tests/csrc/area_through_host_check.cpp).
No sanitizer comes near code loaded into Python: the program has its own main."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import area_ref as AR
import area_through_ref as XR
from area_through_cases import SCENES, arrays, frame_of, moved_mesh_scene
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
NEW = ("srt_area_coverage_through", "srt_area_triangle_coverage_through", "srt_area_coverage_through_device", "srt_select_area_through",
       "srt_group_area_coverage_through", "srt_group_area_triangle_coverage_through", "srt_group_select_area_through", "srt_pick_rays",
       "srt_group_pick_rays")


def test_symbols_signatures_and_sizes():
    lib = T.load_library()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srt_abi.h").read_text(), flags=re.S)
    vp, sz = C.c_void_p, C.c_size_t
    kinds = {"srt_tracer *": vp, "srt_group *": vp, "const srt_render_data *": vp, "const srt_area *": vp, "const int32_t *": vp, "uint32_t *": vp,
             "srt_area_summary *": vp, "const float *": vp, "srt_ray *": vp, "size_t": sz, "uint32_t": C.c_uint32, "int": C.c_int, "size_t *": C.POINTER(sz)}
    for sym in NEW:
        assert sym in T.ABI_SYMBOLS and hasattr(lib, sym), sym
        m = re.search(rf"\bint {sym}\((.*?)\);", header, re.S)
        assert m, sym
        want = []
        for arg in m.group(1).split(","):
            kind = re.sub(r"\w+$", "", " ".join(arg.split())).strip()  # the declaration without the parameter's name
            want.append(kinds[kind])
        got = list(getattr(lib, sym).argtypes)
        assert len(got) == len(want) and all(g is w_ or (g is vp and w_ is vp) for g, w_ in zip(got, want)), (sym, got, want)
    # each through call takes the arguments of its visible counterpart
    for pre in ("srt_", "srt_group_"):
        for name in ("area_coverage", "area_triangle_coverage", "select_area"):
            assert list(getattr(lib, pre + name + "_through").argtypes) == list(getattr(lib, pre + name).argtypes), (pre, name)
    assert list(lib.srt_area_coverage_through_device.argtypes) == list(lib.srt_area_coverage_device.argtypes)
    sizes = (sz * 2)()
    assert lib.srt_area_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (R.AREA.itemsize, R.AREA_SUMMARY.itemsize) == (32, 32)
    assert R.RAY.itemsize == 32
    # NULL handles are refused before anything is touched
    assert lib.srt_area_coverage_through(None, None, None, None, None, 0, None) != 0 and lib.srt_pick_rays(None, None, None, 0, None) != 0
    assert lib.srt_select_area_through(None, None, None, None, 0, 1, None) != 0 and lib.srt_group_pick_rays(None, None, None, 0, None) != 0
    for cls in (T.Tracer, T.TracerGroup):
        assert callable(cls.pick_rays)


class _Recorder(T._Area, T._RayQuery):
    """the shared classes over a handle that records which entry point a call names"""

    def __init__(self):
        self.called, self.options, self.scene_data = [], R.render_data(8, 4), R.scene_data(3)

    def _dn(self, name, *args):
        self.called.append(name)
        return 0

    def _check(self, rc):
        assert rc == 0


def test_the_default_paths_call_the_old_entry_points():
    r = _Recorder()
    r.area_coverage((0, 0, 8, 4))
    r.area_triangle_coverage(1, 12, (0, 0, 8, 4))
    r.select_area((0, 0, 8, 4))
    r.area_coverage((0, 0, 8, 4), through=False)
    assert r.called == ["area_coverage", "area_triangle_coverage", "select_area", "area_coverage"]
    r.called.clear()
    r.area_coverage((0, 0, 8, 4), through=True)
    r.area_triangle_coverage(1, 12, (0, 0, 8, 4), through=True)
    r.select_area((0, 0, 8, 4), [(1, 1), (5, 1), (3, 3)], through=True)
    r.pick_rays([[0.5, 0.5]])
    assert r.called == ["area_coverage_through", "area_triangle_coverage_through", "select_area_through", "pick_rays"]
    import inspect
    for fn in (T._Area.area_coverage, T._Area.area_triangle_coverage, T._Area.select_area, T.Tracer.area_coverage_device):
        assert inspect.signature(fn).parameters["through"].default is False, fn


@pytest.mark.parametrize("name", sorted(SCENES) + ["mesh_moved"])
def test_the_cameras_see_through(name, oracle):
    """with the oracle alone: some pixel has at least 3 candidates and some shape is met on more pixels than it is visible on"""
    scn, rd = (moved_mesh_scene(), frame_of("mesh_smooth")) if name == "mesh_moved" else (arrays(name), frame_of(name))
    w, h = int(rd["width"]), int(rd["height"])
    lists = XR.candidate_lists(oracle, scn, XR.host_rays(rd))
    most, more = XR.sees_through(lists, w, h, len(scn[0]))
    assert most >= 3 and more, (name, most, more)
    if name.startswith("mesh"):
        for s0 in (1, 2):  # a face that is nowhere visible is crossed by some pixel's ray
            n_tri = int(scn[0]["num_triangles"][s0])
            counts, s = XR.triangle_coverage(lists, w, h, s0, n_tri, (0, 0, w, h), None)
            first = np.array([cl[0][2] if cl and cl[0][1] == s0 else -1 for cl in lists])
            vis = np.bincount(first[first >= 0], minlength=n_tri)
            assert ((vis == 0) & (counts > 0)).any() and counts.sum() > s["target_pixels"] == s["hit_pixels"] > 0


def test_the_reference_counts_as_the_definition_says():
    # a 3x2 frame; pixel 0: shape 2 twice (two triangles) behind shape 0; pixel 1: nothing; pixel 4: shape 2 once, shape 5 (beyond a short array)
    lists = [[(1.0, 0, None), (2.0, 2, 7), (2.5, 2, 3)], [], [(1.0, 1, None)], [], [(3.0, 2, 3), (4.0, 5, None)], [(1.0, 5, None)]]
    counts, s = XR.coverage(lists, 3, 2, (0, 0, 3, 2), None, 6)
    assert counts.tolist() == [1, 1, 2, 0, 0, 2] and s == dict(area_pixels=6, hit_pixels=4, miss_pixels=2, distinct=4, target_pixels=0)
    counts, s = XR.coverage(lists, 3, 2, (0, 0, 3, 2), None, 3)  # shape 5 is beyond the array: dropped from counts, its pixels still hits
    assert counts.tolist() == [1, 1, 2] and s == dict(area_pixels=6, hit_pixels=4, miss_pixels=2, distinct=3, target_pixels=0)
    counts, s = XR.coverage(lists, 3, 2, (1, 0, 9, 1), None, 6)
    assert counts.tolist() == [0, 1, 0, 0, 0, 0] and s == dict(area_pixels=2, hit_pixels=1, miss_pixels=1, distinct=1, target_pixels=0)
    counts, s = XR.triangle_coverage(lists, 3, 2, 2, 8, (0, 0, 3, 2), None)
    assert counts.tolist() == [0, 0, 0, 2, 0, 0, 0, 1] and s == dict(area_pixels=6, hit_pixels=2, miss_pixels=4, distinct=2, target_pixels=2)
    assert counts.sum() == 3 > s["target_pixels"]  # target_pixels counts pixels, not crossings
    assert XR.visible(lists, 3, 2, 6).tolist() == [[0, AR.NONE, 1], [AR.NONE, 2, 5]]
    assert XR.sees_through(lists, 3, 2, 6) == (3, [2, 5])
    bad = np.zeros(3, R.RAY)
    bad["direction"][:, 2], bad["tmax"] = -1.0, np.inf
    bad["origin"][1, 0], bad["direction"][2] = np.nan, 0.0
    assert [XR.ray_valid(r) for r in bad] == [True, False, False]
    assert np.array_equal(XR.pixel_centres(3, 2), np.asarray([[0.5, 0.5], [1.5, 0.5], [2.5, 0.5], [0.5, 1.5], [1.5, 1.5], [2.5, 1.5]], np.float32))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stand_alone_grid_check_under_sanitizers(tmp_path):
    """tests/csrc/area_through_host_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program of its own: no
    report, exit status 0, and the grids it prints equal the arithmetic restated here."""
    csrc = ROOT / "simple-raytracer_amd" / "csrc"
    exe, cases_file = tmp_path / "area_through_host_check", tmp_path / "cases.txt"
    cases = [(w, h, AR.RECTS[n]) for n in sorted(AR.RECTS) for (w, h) in ((AR.W, AR.H), (1, 1), (3, 2), (130, 6))]
    cases += [(130, 6, r) for r in ((0, 0, 64, 4), (0, 0, 65, 5), (1, 1, 64, 2), (66, 1, 130, 5), (-(1 << 31), -(1 << 31), (1 << 31) - 1, (1 << 31) - 1))]
    cases_file.write_text("".join(f"{w} {h} {r[0]} {r[1]} {r[2]} {r[3]}\n" for w, h, r in cases))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           f"-I{csrc}", str(ROOT / "tests/csrc/area_through_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(cases_file)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-400:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == len(cases) + 1
    for (w, h, rect), line in zip(cases, lines):
        x0, y0, x1, y1 = max(0, min(rect[0], w)), max(0, min(rect[1], h)), max(0, min(rect[2], w)), max(0, min(rect[3], h))
        x1, y1 = max(x1, x0), max(y1, y0)
        empty = x0 >= x1 or y0 >= y1
        cg, rg = (0, 0) if empty else ((x1 - x0 + 63) // 64, (y1 - y0 + 3) // 4)
        assert line == f"{x0} {y0} {x1} {y1} {cg} {rg} {cg * rg}", (w, h, rect, line)
