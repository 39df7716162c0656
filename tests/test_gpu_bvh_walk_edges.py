"""GPU: the directed cases of tests/bvh_walk_cases.py through every compiled instantiation of walk_bvh -- the plain BVH kernel,
the triangle-counting one, the textured twin of kernels_tex.hip -- over the host's SAH tree and the device's median-order tree.
Origins exactly on decoded planes of child boxes (the entry distance before the clamp is -0.0 there: fmaxf(-0.0f, 0.0f) must be
+0 or the child's key passes SRT_BVH_KEY_INF), one ulp to either side, fans into, out of and in the plane, axis-parallel rays
with +0 and -0 components over vertices, edges and box edges, rays in a flat sheet's own plane. Every frame: the canvas of
the array scan bit for bit, its ray, sky, path and NaN-pixel counts, no watchdog; in every configuration a subset per family is
the CPU oracle's too (the textured oracle's under the textured kernels, whose 1x1 texture is not white).
One scan handle and one BVH handle per mesh; only the camera changes between frames (4x2 pixels, 1 or 2 samples)."""
import numpy as np
import pytest

import bvh_walk_cases as W
import texture_cases as TC
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu
DEVICE, MEDIAN = 1, 1  # SRT_BUILD_DEVICE, SRT_BUILD_ORDER_MEDIAN
CONFIGS = ["plain", "count", "textured"]
NON_VACUOUS = ("on_plane_in", "axis_parallel")
ORACLE_PER_MESH_AND_TREE = 10  # of each family: 20 frames and more in every test (in_plane_grazing has the two grid meshes only)


def handle(T, sky, sc, config, accel, kind="sah", shapes=None):
    shapes = sc["shapes"] if shapes is None else shapes
    t = T.Tracer(W.W, W.H)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    if accel and kind == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    if config == "count":
        t.count_triangles(True)
    if config == "textured":  # a 1x1 texture on both materials: the textured kernels run
        t.set_textures([W.TEXTURE])
        t.set_material_textures(W.texture_bindings())
    t.options = R.render_data(W.W, W.H, 1, 1)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, sc["tris"], sc["mats"])
    return t


def frame(t, rec, show_normals=None):
    t.options = W.render_data(rec, show_normals)
    t.clear_canvas()
    t.reset_counters()
    t.trace()
    return t.read_canvas(), t.counters()


@pytest.mark.parametrize("kind", W.TREES)
@pytest.mark.parametrize("config", CONFIGS)
def test_walk_equals_scan_on_the_directed_cases(config, kind, T, sky, oracle):
    failures, n_frames = [], 0
    hit_cases = {fam: [0, 0] for fam in NON_VACUOUS}
    oracle_frames = {fam: 0 for fam in W.FAMILIES}
    for mesh in W.MESH_NAMES:
        sc, tr = W.scene(mesh), W.tree(mesh, kind)
        scan, bvh = handle(T, sky, sc, config, 0), handle(T, sky, sc, config, 1, kind)
        table = TC.oracle_table((sc["shapes"], sc["tris"], sc["mats"]), [W.TEXTURE], W.texture_bindings())
        alone = handle(T, sky, sc, config, 0, shapes=sc["shapes"][1:])  # the sphere without the model: what a frame shows where no ray hits the model
        # the device walks the planes the cases were aimed at
        inner = tr["wide"]["blocks"][:, 3] != 0
        blocks = bvh.read_bvh_blocks()
        assert blocks.shape == tr["wide"]["blocks"].shape and np.array_equal(blocks[inner, :12], tr["wide"]["blocks"][inner, :12])
        if kind == "median":
            assert bvh.acceleration_build_info()["models"] == 1
        for fam, recs in W.cases(mesh, kind).items():
            with_oracle = {rec["name"] for rec in W.oracle_subset(mesh, kind, fam, ORACLE_PER_MESH_AND_TREE)}
            for rec in recs:
                normals = False if config == "textured" else None  # (show_normals frames take the untextured kernels: every case runs the twin)
                want, wc = frame(scan, rec, normals)
                got, gc = frame(bvh, rec, normals)
                n_frames += 1
                if config == "textured":
                    assert scan.last_trace_textured() and bvh.last_trace_textured()
                same = bits_equal(got, want) and all(gc[k] == wc[k] for k in ("rays", "sky", "paths", "nan_pixels")) and gc["watchdog"] == 0 and wc["watchdog"] == 0
                if not same:
                    failures.append((rec["name"], "scan"))
                if rec["name"] in with_oracle:
                    with np.errstate(all="ignore"):
                        if config == "textured":  # the textured oracle (tests/test_oracle_textures.py), as tests/test_gpu_texture_paths.py
                            o = oracle.render_textured(W.render_data(rec, normals), scan.scene_data, sc["shapes"], sc["tris"], sc["mats"], sky, table)
                        else:
                            o = oracle.render(W.render_data(rec), scan.scene_data, sc["shapes"], sc["tris"], sc["mats"], sky)
                    oracle_frames[fam] += 1
                    if not bits_equal(want, o):
                        failures.append((rec["name"], "oracle"))
                if fam in NON_VACUOUS:
                    seen, _ = frame(scan, rec, show_normals=True)
                    empty, _ = frame(alone, rec, show_normals=True)
                    hit_cases[fam][0] += int(not bits_equal(seen, empty))
                    hit_cases[fam][1] += 1
        for t in (scan, bvh, alone):
            t.close()
    print(f"{n_frames} frames, model hit in {hit_cases}, oracle frames {oracle_frames}")
    assert not failures, failures
    for fam, (hit, n) in hit_cases.items():
        assert 2 * hit >= n, (fam, hit, n)
    assert all(n >= 20 for n in oracle_frames.values()), oracle_frames
