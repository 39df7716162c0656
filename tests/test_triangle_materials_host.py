"""CPU: per-triangle materials (include/srt_abi.h "per-triangle materials"). What earns the split-scene oracle its trust
(tests/triangle_material_cases.py), the coverage of every view tests/test_gpu_triangle_materials.py renders, the host-only
check of a table, and the OBJ `usemtl` / MTL side of host/parser.hpp -- driven by a stand-alone program
(tests/csrc/parser_materials_check.cpp) that is built with -fsanitize=address,undefined and by srt_headless --obj-materials."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import texture_cases as TC
import triangle_material_cases as M
from conftest import ROOT, bits_equal
from simple_raytracer_amd import records as R

SRT_OK, SRT_ERR_INVALID = 0, 1


def share_differing(a, b):
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).mean())


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unsplit(oracle, sky):
    return {name: TC.oracle_path_canvas(oracle, sky, TC.path_case(name)) for name in ("mesh", "big")}


@pytest.mark.parametrize("run", [1, 5])
@pytest.mark.parametrize("name", ["mesh", "big"])
def test_split_is_neutral(oracle, sky, unsplit, name, run):
    """Runs that keep their shape's material: the textured oracle's canvas (LINEAR, with UVs, ten bounces) does not change by
    a bit. Scan order, the tie rule, the triangle index that selects UVs and the RNG stream survive the split."""
    case = TC.path_case(name)
    shapes, tris, mats = case["scn"]
    split, origin = M.split_by_run_length(shapes, run)
    n_model_tris = int(shapes["num_triangles"][shapes["type"] == R.SHAPE_MODEL].sum())
    if run == 1:
        assert len(split) == int((shapes["type"] != R.SHAPE_MODEL).sum()) + n_model_tris
    assert len(split) > len(shapes) and np.array_equal(np.unique(origin), np.arange(len(shapes)))
    assert np.array_equal(split["material"], shapes["material"][origin])
    case = dict(case, scn=(split, tris, mats))
    got = TC.oracle_path_canvas(oracle, sky, case, *TC.case_render_data(case))
    assert bits_equal(got, unsplit[name])


def test_split_by_table_shapes():
    """the split itself: runs, ranges and materials; -1 and a shape without a material keep the shape's"""
    shapes, tris, mats = TC.mesh_path_scene()
    shapes = shapes.copy()
    shapes["material"][3] = -1  # the third instance (over triangles 0..11): a miss whatever its triangles say
    tm = np.full(len(tris), -1, np.int32)
    tm[2:5] = 1
    tm[5] = 0  # the shape's own material by name: one run with what follows
    tm[11] = 2
    split, origin = M.split_by_triangle_materials(shapes, tm)
    assert origin.tolist() == [0, 0, 0, 0, 1, 2, 3]
    assert split["triangle_index"][:4].tolist() == [0, 2, 5, 11] and split["num_triangles"][:4].tolist() == [2, 3, 6, 1]
    assert split["material"].tolist() == [0, 1, 0, 2, 1, 2, -1]
    assert split["num_triangles"][5] == 12 and split["num_triangles"][6] == 12
    for k in (0, 1, 2, 3):
        assert np.array_equal(split["transform"][k], shapes["transform"][0]) and np.array_equal(split["bounding_min"][k], shapes["bounding_min"][0])


@pytest.mark.parametrize("view", M.GPU_VIEWS, ids=lambda v: "-".join(str(x) for x in v))
def test_coverage_of_gpu_views(oracle, sky, view):
    """On every view the GPU tests hold to the split oracle, the table changes at least a fifth of the oracle's pixels."""
    name, assignment, textured, w, h = view
    case = M.tm_case(name, assignment, textured, w, h)
    share = share_differing(M.oracle_canvas(oracle, sky, case), M.oracle_canvas(oracle, sky, case, tm=None))
    print(view, f"{share:.3f} of the pixels differ")
    assert share >= 0.2, (view, share)


@pytest.mark.parametrize("view", M.SPECIAL_VIEWS, ids=lambda v: "-".join(str(x) for x in v))
def test_coverage_of_special_views(oracle, sky, view):
    name, assignment, textured, w, h = view
    case = M.tm_case(name, assignment, textured, w, h)
    with_table, without = M.oracle_canvas(oracle, sky, case), M.oracle_canvas(oracle, sky, case, tm=None)
    if assignment == "all_minus_one":
        assert bits_equal(with_table, without)
    else:
        assert int((case["tm"] >= 0).sum()) == 1 and share_differing(with_table, without) > 0.0


def test_fuzz_cases_are_what_they_say():
    for seed in M.FUZZ_SEEDS:
        case = M.fuzz_case(seed)
        shapes, tris, mats = case["scn"]
        models = shapes[shapes["type"] == R.SHAPE_MODEL]
        assert len(models) == 3 and all(12 <= int(n) <= 40 for n in models["num_triangles"])
        tm = case["tm"]
        assert len(tm) == len(tris) and tm.min() >= -1 and tm.max() < len(mats)
        assert (mats["transmittance"] > 0).any() and (mats["emission_strength"] > 0).any()
    share = np.mean([float((M.fuzz_case(s)["tm"] < 0).mean()) for s in M.FUZZ_SEEDS])
    assert 0.25 < share < 0.42  # a third of the entries -1


# ---- srt_triangle_materials_check_host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_host():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer.triangle_materials_check_host


def test_check_host(check_host):
    ok = np.array([-1, 0, 2, -1, 1], np.int32)
    assert check_host(ok, 5, 3) == SRT_OK
    assert check_host(ok, 4, 3) == SRT_ERR_INVALID and check_host(ok, 6, 3) == SRT_ERR_INVALID  # wrong count
    assert check_host(np.array([-1, -2, 0], np.int32), 3, 3) == SRT_ERR_INVALID  # below -1
    assert check_host(np.array([0, 3, 0], np.int32), 3, 3) == SRT_ERR_INVALID  # == n_materials
    assert check_host(np.array([0, 2, 0], np.int32), 3, 3) == SRT_OK
    assert check_host(np.array([-1, -1], np.int32), 2, 0) == SRT_OK  # no materials, nothing names one
    assert check_host(np.array([-1, 0], np.int32), 2, 0) == SRT_ERR_INVALID
    assert check_host(None, 7, 3) == SRT_OK  # NULL with 0: no table
    assert check_host(None, 0, 0) == SRT_OK


# ---- the parser ------------------------------------------------------------------------------------------------------------------
OBJ = """mtllib six.mtl
v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
vt 0.25 0.75
f 1 2 3
f 1/1 2/1 4/1
usemtl red
f 1 3 4
usemtl glass
f 2 3 4
f 3 2 1
usemtl red
f 4 2 1
usemtl nowhere
f 4 3 1
"""
MTL = """# six materials
Kd 9 9 9
newmtl red
Kd 0.8 0.1 0.1
Ns 500
newmtl glass
d 0.25
Ni 1.5
Ns 900
Pr 0.1
newmtl also_glass
Tr 0.25
Pr 0.3
Ns 100
unknown_key 1 2 3
newmtl lamp
Ke 0 0.5 0
Ns 2500
newmtl metal
Pm 0.6
Ke 0 0 0
Ns -5
map_Kd -s 2 2 2 wood.ppm
newmtl plain
illum 2
"""


@pytest.fixture(scope="module")
def parser_check(tmp_path_factory):
    """tests/csrc/parser_materials_check.cpp with its own main, built with the host compiler and both sanitisers"""
    exe = tmp_path_factory.mktemp("parser") / "parser_materials_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        str(ROOT / "tests" / "csrc" / "parser_materials_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "six.mtl").write_text(MTL)
    return tmp_path


def run_check(exe, *paths):
    r = subprocess.run([exe, *map(str, paths)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_obj_usemtl_groups(parser_check, files):
    out = run_check(parser_check, files / "m.obj")
    assert out[0][0] == "obj" and out[0][2] == "ok"
    assert out[1] == ["range", "2", "7"]  # appended behind the two triangles that were there
    assert out[2] == ["names", "red", "glass", "nowhere"]  # in order of first use, each once
    assert out[3] == ["faces", "-1", "-1", "0", "1", "1", "0", "2"]  # two faces before any usemtl; red comes back
    assert out[4] == ["mtllibs", "six.mtl"]
    assert out[5] == ["plain", "same"]  # without the new arguments: the triangles and UVs it returned before


def test_load_mtl_mapping(parser_check, files):
    out = run_check(parser_check, files / "six.mtl", files / "missing.mtl")
    assert out[0][0] == "mtl" and out[0][2] == "6" and out[-1][0] == "mtl" and out[-1][2] == "0"  # a missing file: an empty list
    got = {l[1]: ([float(x) for x in l[2:14]], l[14]) for l in out if l[0] == "material"}
    f = lambda x: float(np.float32(x))
    # smoothness metallic specular emission_strength transmittance refraction_index | colour | emission | map_Kd
    want = {
        "red": ([f(np.float32(500) / np.float32(1000)), 0, 0, 0, 0, 1, f(0.8), f(0.1), f(0.1), 0, 0, 0], "-"),        # Ns without Pr
        "glass": ([f(np.float32(1) - np.float32(0.1)), 0, 0, 0, f(np.float32(1) - np.float32(0.25)), 1.5, 1, 1, 1, 0, 0, 0], "-"),  # d; Pr wins over an earlier Ns
        "also_glass": ([f(np.float32(1) - np.float32(0.3)), 0, 0, 0, 0.25, 1, 1, 1, 1, 0, 0, 0], "-"),               # Tr; a later Ns is ignored
        "lamp": ([1, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0.5, 0], "-"),                                                      # Ke > 0: strength 1; Ns clamped
        "metal": ([0, f(0.6), 0, 0, 0, 1, 1, 1, 1, 0, 0, 0], "wood.ppm"),                                             # Ke 0: strength 0; Ns clamped at 0
        "plain": ([0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0], "-"),                                                       # Material()'s defaults
    }
    assert list(got) == list(want)  # file order
    for name in want:
        assert got[name][1] == want[name][1], name
        assert np.array_equal(np.array(got[name][0], np.float32), np.array(want[name][0], np.float32)), (name, got[name][0])


def test_parser_under_sanitisers_on_truncated_files(parser_check, files):
    """the same program (address and undefined-behaviour sanitisers) on the files above cut short at every length that ends
    inside a token, on an OBJ whose indices point nowhere, and on empty files"""
    paths = []
    for k, cut in enumerate([len(OBJ) - 3, len(OBJ) // 2, 40, 17]):
        p = files / f"cut{k}.obj"
        p.write_text(OBJ[:cut])
        paths.append(p)
    for k, cut in enumerate([len(MTL) - 9, len(MTL) // 2, 25]):
        p = files / f"cut{k}.mtl"
        p.write_text(MTL[:cut])
        paths.append(p)
    (files / "bad.obj").write_text("usemtl\nusemtl a\nv 0 0 0\nf 1 2 3\nf 1/9/9 1 1\nmtllib\n")
    (files / "empty.obj").write_text("")
    (files / "empty.mtl").write_text("")
    out = run_check(parser_check, *paths, files / "bad.obj", files / "empty.obj", files / "empty.mtl", files / "m.obj", files / "six.mtl")
    objs = [l for l in out if l[0] == "obj"]
    assert [l[2] for l in objs] == ["ok", "ok", "ok", "ok", "none", "ok", "ok"]  # bad.obj: an index beyond the vertices
    assert all(l[1] == "same" for l in out if l[0] == "plain")


# ---- srt_headless --obj-materials ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def headless():
    from simple_raytracer_amd import build
    return str(build.build_headless())


def test_headless_obj_materials_parse_only(headless, files):
    prefix = str(files / "d")
    r = subprocess.run([headless, "--scene", "meshes", "--obj", str(files / "m.obj"), "--obj-materials", "--parse-only", "--dump", prefix],
                       capture_output=True, text=True, check=True)
    mats, tris = np.fromfile(prefix + ".mats.bin", R.MATERIAL), np.fromfile(prefix + ".tris.bin", R.TRIANGLE)
    tm = np.fromfile(prefix + ".tm.bin", np.int32)
    assert len(mats) == 3 + 6 and len(tris) == 12 + 7 and len(tm) == len(tris)
    # the scene's three materials, then six.mtl's in file order: red = 3, glass = 4; `nowhere` has no MTL entry
    assert tm.tolist() == [-1] * 12 + [-1, -1, 3, 4, 4, 3, -1]
    assert np.array_equal(mats["color"][3], np.array([0.8, 0.1, 0.1], np.float32)) and mats["transmittance"][4] == np.float32(0.75)
    assert "per-triangle materials: 19 triangles, 4 with a material of their own, 3 usemtl names: red=3 glass=4 nowhere=-1" in r.stdout
    assert "wood.ppm" not in r.stderr  # (textures are read when there is a tracer to hand them to)
    # off by default: the same invocation without the switch dumps what it dumped before
    subprocess.run([headless, "--scene", "meshes", "--obj", str(files / "m.obj"), "--parse-only", "--dump", prefix + "0"], check=True)
    assert len(np.fromfile(prefix + "0.mats.bin", R.MATERIAL)) == 3 and not Path(prefix + "0.tm.bin").exists()
    tris0, shapes0, shapes = np.fromfile(prefix + "0.tris.bin", R.TRIANGLE), np.fromfile(prefix + "0.shapes.bin", R.SHAPE), np.fromfile(prefix + ".shapes.bin", R.SHAPE)
    assert np.array_equal(tris0["v"]["pos"], tris["v"]["pos"]) and np.array_equal(tris0["v"]["normal"], tris["v"]["normal"])
    assert np.array_equal(shapes0["type"], shapes["type"]) and np.array_equal(shapes0["material"], shapes["material"])
    models = shapes["type"] == R.SHAPE_MODEL  # (the other kinds leave the model's part of the union as it was)
    for field in ("triangle_index", "num_triangles", "transform", "bounding_min", "bounding_max"):
        assert np.array_equal(shapes0[field][models], shapes[field][models]), field
