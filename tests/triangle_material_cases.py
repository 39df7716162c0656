"""What the per-triangle material tests share (tests/test_triangle_materials_host.py, tests/test_gpu_triangle_materials.py): the
split of a scene into runs -- the oracle of srt_set_triangle_materials -- the assignments, the cases built on
texture_cases.path_case and the seeded fuzz scenes. A plain module, not a test module.

THE ORACLE. A model whose triangles carry materials renders the same canvas as the same model split into one model shape per
maximal run of consecutive triangles with the same effective material: each run shape keeps the original's transform and
bounds and its place in the shape array, and takes `triangle_index + start`, the run's length and the run's material. Scan
order, the `t < tmin` tie rule, the global triangle index that selects UVs and the RNG stream do not change with the split
(tests/test_triangle_materials_host.py holds the neutral half of this -- runs that keep the shape's material -- bit for
bit), so oracle/ is used as it is, on the split scene."""
import numpy as np

import texture_cases as TC
import texture_ref as TR
from simple_raytracer_amd import records as R

F = np.float32


# ---- the split --------------------------------------------------------------------------------------------------------------
def effective_materials(shapes, s, tm):
    """the material of every triangle of model shape s under table tm (None: none): the table's entry where it is >= 0 and the
    shape has a material, else the shape's"""
    ti, n, m = int(shapes["triangle_index"][s]), int(shapes["num_triangles"][s]), int(shapes["material"][s])
    eff = np.full(n, m, np.int64)
    if tm is not None and m >= 0:
        e = np.asarray(tm, np.int64)[ti:ti + n]
        eff = np.where(e >= 0, e, m)
    return eff


def _split(shapes, keys_of, material_of):
    """One shape per maximal run of equal keys (keys_of(s) -> one key per triangle of model s); material_of(s, key) -> the run's
    material. -> (shapes, origin): origin[i] = the index in `shapes` of the shape that run shape i came from."""
    raw = np.ascontiguousarray(shapes).view(np.uint8).reshape(len(shapes), R.SHAPE.itemsize)
    rows, origin, patch = [], [], []
    for s in range(len(shapes)):
        n = int(shapes["num_triangles"][s]) if shapes["type"][s] == R.SHAPE_MODEL else 0
        if n == 0:
            rows.append(raw[s]), origin.append(s), patch.append(None)
            continue
        keys = np.asarray(keys_of(s))
        ti, start = int(shapes["triangle_index"][s]), 0
        for k in range(1, n + 1):
            if k == n or keys[k] != keys[start]:
                rows.append(raw[s]), origin.append(s), patch.append((ti + start, k - start, material_of(s, keys[start])))
                start = k
    out = np.frombuffer(np.stack(rows).tobytes(), R.SHAPE).copy() if rows else np.zeros(0, R.SHAPE)
    for i, p in enumerate(patch):
        if p is not None:
            out["triangle_index"][i], out["num_triangles"][i], out["material"][i] = p
    return out, np.asarray(origin, np.int64)


def split_by_triangle_materials(shapes, tm):
    """the split scene of table tm -> (shapes, origin)"""
    return _split(shapes, lambda s: effective_materials(shapes, s, tm), lambda s, key: int(key))


def split_by_run_length(shapes, run):
    """the neutral split: runs of `run` triangles that keep their shape's material -> (shapes, origin)"""
    return _split(shapes, lambda s: np.arange(int(shapes["num_triangles"][s])) // run, lambda s, key: int(shapes["material"][s]))


# ---- assignments ----------------------------------------------------------------------------------------------------------------
def per_face(n_triangles, n_materials):
    """a material per face of a box (two triangles), every fifth entry -1"""
    k = np.arange(n_triangles)
    return np.where(k % 5 == 4, -1, (k // 2) % n_materials).astype(np.int32)


def interleaved(n_triangles, n_materials):
    """every run has length 1"""
    return (np.arange(n_triangles) % n_materials).astype(np.int32)


def all_minus_one(n_triangles, n_materials):
    return np.full(n_triangles, -1, np.int32)


# the one entry >= 0 of the single-entry tables: (triangle, material), a triangle the camera of the case sees (the host tests
# assert that the oracle's canvas changes with it)
SINGLE = {"mesh": (2, 1), "mesh_pad": (2, 1), "big": (40, 4)}


def single(name):
    def make(n_triangles, n_materials):
        tm = np.full(n_triangles, -1, np.int32)
        tm[SINGLE[name][0]] = SINGLE[name][1]
        return tm
    return make


ASSIGNMENTS = {"per_face": per_face, "interleaved": interleaved, "all_minus_one": all_minus_one}
PAD_FIRST = 40  # mesh_pad: materials[40..43] are the mesh's four again, far beyond the LDS copy's reach of a small scene


def tm_case(name, assignment, textured=True, w=37, h=29):
    """texture_cases.path_case(name) (LINEAR, with UVs) with a table: case["tm"]. name: mesh, big, or mesh_pad -- mesh with 80
    more materials (the scene records leave LDS), four of them (PAD_FIRST..) copies of the mesh's own, which the table points
    at instead of 0..3. assignment: a key of ASSIGNMENTS, "single", or an array. textured=False: no image, no binding, no UVs
    -- the table alone reaches the textured kernels."""
    case = dict(TC.path_case("mesh" if name == "mesh_pad" else name, TR.LINEAR, True, w=w, h=h))
    shapes, tris, mats = case["scn"]
    n_own = len(mats)
    if name == "mesh_pad":
        mats = R.concat(R.MATERIAL, mats, np.zeros(80, R.MATERIAL))
        mats[PAD_FIRST:PAD_FIRST + n_own] = mats[:n_own]
        case["scn"] = (shapes, tris, mats)
        case["bindings"] = R.concat(R.MATERIAL_TEXTURE, case["bindings"], np.array([R.material_texture()] * 80, R.MATERIAL_TEXTURE))
        case["bindings"][PAD_FIRST:PAD_FIRST + n_own] = case["bindings"][:n_own]
    if isinstance(assignment, str):
        make = single(name) if assignment == "single" else ASSIGNMENTS[assignment]
        tm = make(len(tris), n_own)
    else:
        tm = np.asarray(assignment, np.int32)
    if name == "mesh_pad":
        tm = np.where(tm >= 0, tm + PAD_FIRST, -1).astype(np.int32)
    case["tm"] = tm
    if not textured:
        case.update(images=[], bindings=None, uvs=None)
    return case


def oracle_canvas(oracle, sky, case, rd=None, sd=None, tm="case", counters=False):
    """The expected canvas of a case: the textured oracle (the plain one without textures) over the split scene. tm: the
    table ("case": the case's own; None: no table, the scene as it is)."""
    if rd is None:
        rd, sd = TC.case_render_data(case)
    shapes, tris, mats = case["scn"]
    split, _ = split_by_triangle_materials(shapes, case["tm"] if isinstance(tm, str) else tm)
    sd = np.array(sd, R.SCENE_DATA).copy()
    sd["num_shapes"] = len(split)
    if case["bindings"] is None:
        return oracle.render(rd, sd, split, tris, mats, sky, counters=counters)
    table = TC.oracle_table((split, tris, mats), case["images"], case["bindings"], case["uvs"])
    return oracle.render_textured(rd, sd, split, tris, mats, sky, table, counters=counters)


def oracle_features(oracle, case, rd, sd, fs):
    """normal_depth, albedo_hits of the feature pass over the split scene"""
    shapes, tris, mats = case["scn"]
    split, _ = split_by_triangle_materials(shapes, case["tm"])
    sd = np.array(sd, R.SCENE_DATA).copy()
    sd["num_shapes"] = len(split)
    if case["bindings"] is None:
        return oracle.features(rd, sd, split, tris, mats, fs)
    table = TC.oracle_table((split, tris, mats), case["images"], case["bindings"], case["uvs"])
    return oracle.features_textured(rd, sd, split, tris, mats, table, fs)


# every (name, assignment, textured, w, h) tests/test_gpu_triangle_materials.py renders against the split oracle;
# tests/test_triangle_materials_host.py asserts the coverage condition on each of them
GPU_VIEWS = ([("mesh", a, tex, w, h) for a in ("per_face", "interleaved") for tex in (True, False) for w, h in TC.FRAMES]
             + [("big", "interleaved", True, 64, 40), ("mesh_pad", "per_face", True, 37, 29), ("mesh_pad", "per_face", False, 37, 29)])
SPECIAL_VIEWS = [("mesh", "all_minus_one", False, 37, 29), ("mesh", "single", False, 37, 29), ("mesh", "single", True, 37, 29)]


# ---- the fuzz scenes ---------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = list(range(40))
FUZZ_W, FUZZ_H, FUZZ_SPP = 16, 12, 2


def _soup(rng, n):
    """n random triangles in [-1, 1]^3, each with its geometric normal or (every third) random vertex normals"""
    t = np.zeros(n, R.TRIANGLE)
    c = rng.uniform(-0.7, 0.7, (n, 1, 3))
    pos = (c + rng.uniform(-0.6, 0.6, (n, 3, 3))).astype(F)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)
    vn = np.repeat(nrm[:, None, :], 3, axis=1)
    smooth = np.arange(n) % 3 == 0
    rnd = rng.normal(size=(n, 3, 3))
    vn[smooth] = (vn + 0.4 * rnd / np.linalg.norm(rnd, axis=2, keepdims=True))[smooth]
    vn = vn / np.linalg.norm(vn, axis=2, keepdims=True)
    t["v"]["pos"], t["v"]["normal"] = pos, vn.astype(F)
    return t


def fuzz_case(seed):
    """Two random meshes of 12 to 40 triangles (one with a second instance), a floor and a sphere; eight random materials, glass
    and emitters among them; a random table with a third of its entries -1. Odd seeds bind textures (no UVs)."""
    rng = np.random.default_rng(9000 + seed)
    na, nb = (int(x) for x in rng.integers(12, 41, 2))
    tris = R.concat(R.TRIANGLE, _soup(rng, na), _soup(rng, nb))
    mats = np.zeros(8, R.MATERIAL)
    for i in range(8):
        kind = i if i < 4 else int(rng.integers(0, 4))  # diffuse, glass, metal / coat, emitter: each at least once
        col = rng.uniform(0.2, 1.0, 3)
        if kind == 0:
            mats[i] = R.material(col)
        elif kind == 1:
            mats[i] = R.material(col, smoothness=rng.uniform(0.7, 1.0), transmittance=rng.uniform(0.5, 1.0), refraction_index=rng.uniform(1.1, 1.7))
        elif kind == 2:
            mats[i] = R.material(col, smoothness=rng.uniform(0.0, 1.0), metallic=rng.uniform(0.0, 1.0), specular=rng.uniform(0.0, 0.6))
        else:
            mats[i] = R.material(col, emission=rng.uniform(0.0, 1.0, 3), emission_strength=rng.uniform(0.5, 3.0))
    xf = lambda: R.mat_mul(R.translate(rng.uniform(-1.2, 1.2, 3) * (1.0, 0.4, 1.0)), R.mat_mul(R.euler_yxz(*rng.uniform(-1.0, 1.0, 3)), R.scale_matrix(rng.uniform(0.6, 1.4, 3))))
    shapes = np.zeros(5, R.SHAPE)
    shapes[0] = R.model(int(rng.integers(0, 8)), tris, 0, na, xf())
    shapes[1] = R.plane(int(rng.integers(0, 8)), (0.0, -1.3, 0.0), (0.0, 1.0, 0.0))
    shapes[2] = R.model(int(rng.integers(0, 8)), tris, na, nb, xf())
    shapes[3] = R.sphere(int(rng.integers(0, 8)), (1.6, 0.2, -1.0), 0.5)
    shapes[4] = R.model(int(rng.integers(-1, 8)), tris, 0, na, xf())  # a second instance; now and then without a material: a miss
    tm = rng.integers(0, 8, na + nb).astype(np.int32)
    tm[rng.random(na + nb) < 1.0 / 3.0] = -1
    textured = seed % 2 == 1
    return dict(scn=(shapes, tris, mats), cam=R.camera_matrix((0.0, 0.3, 3.2), 0.0, -0.1), tm=tm, w=FUZZ_W, h=FUZZ_H, spp=FUZZ_SPP, bounces=10,
                time=1000 + 17 * seed, images=TC.PATH_TEXTURES if textured else [], uvs=None,
                bindings=TC.path_bindings(8, TR.LINEAR if seed % 4 == 1 else TR.NEAREST, first=seed) if textured else None)
