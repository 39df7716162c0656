"""The differential fuzz's scene generators, the lanes that aim them at every trace kernel the library launches, and a
restatement of the library's choice of kernel. A plain module, not a test module: tests/test_gpu_fuzz.py, test_gpu_bvh.py,
test_gpu_fuzz_dispatch.py, test_fuzz_lanes.py and the soak scripts import it.

random_scene() is the generator of tests/test_gpu_fuzz.py, moved here unchanged: the same RNG calls in the same order.

A LANE is a generator of (shapes, tris, mats, cam, rd, sd, expected, extra): expected = (scene class, textured) the library
must report for the dispatch (Tracer.last_trace_class / last_trace_textured), BY CONSTRUCTION of the lane; extra = what the
runner needs besides (acceleration mode, textures, the near-miss edit). expected_class() is the independent restatement of
csrc/srt_abi.hip scene_class() from the rules (block building as csrc/scene_prep.cpp does it, one group, LDS fit, thresholds by their definition); the tests
demand lane intention == restatement == library.

  class1..class4  one per entry of device_types.h SRT_SCENE_CLASS_LIST, everything else random; the hostile flavour draws only
                  values that keep the scene in its class
  near_miss       a class scene with exactly one edit that must send it to the general kernel (or to the other PPS class)
  scan, bvh, scan_pad, bvh_pad, shapes_only
                  random_scene as the product runs it (count_triangles off): array scan and BVH, each also with 80 zero
                  materials appended (the scene records no longer fit LDS), and a sphere / plane scene of several block groups
  tex_*           the same scenes with every material bound NEAREST to a texture whose texels all equal its colour: the
                  textured twins must give the UNTEXTURED oracle's canvas
  texvar_*        the tex_* scenes with images of 1x1 to 5x4 random texels (finite, not negative) and random filters: the
                  textured twins must give the TEXTURED oracle's canvas (oracle/srt_oracle.c orc_render_textured)
"""
import numpy as np

import texture_cases
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
GENERAL, PPS, PPS_SPECULAR, SSS, PPP = 0, 1, 2, 3, 4  # device_types.h SRT_SCENE_CLASS_LIST
ACCEL_NONE, ACCEL_BVH = 0, 1
NEAREST = 1
LINEAR = 0
MAX_TEXTURES = 64
PAD_MATERIALS = 80  # 80 more 64-byte materials: no scene fits the 4608-byte LDS copy
FRAME = (23, 17)  # ragged: 391 pixels, the last wave is partial


def random_scene(rng, hostile):
    n_mats = rng.randint(1, 7)
    mats = np.zeros(n_mats, R.MATERIAL)
    for i in range(n_mats):
        mats[i] = R.material(rng.uniform(0, 1, 3), smoothness=rng.uniform(0, 1), metallic=rng.choice([0, 0, 1, rng.uniform()]),
                             specular=rng.choice([0, 0, rng.uniform()]), transmittance=rng.choice([0, 0, 1, rng.uniform()]),
                             refraction_index=rng.choice([1.0, 1.5, 1.33, rng.uniform(0.5, 2.5)]),
                             emission=rng.uniform(0, 1, 3), emission_strength=rng.choice([0, 0, rng.uniform(0, 5)]))
    if hostile:
        m = mats[rng.randint(n_mats)]
        kind = rng.randint(8)
        if kind == 6: m["metallic"] = rng.choice([1.5, -0.2, np.inf])      # probabilities outside [0, 1]: the integer-threshold
        if kind == 7: m["transmittance"], m["specular"] = 2.0, -1.0        # draws (device_math.h bernoulli) fall back to floats
        if kind == 0: m["refraction_index"] = 0.0
        if kind == 1: m["color"] = (np.nan, 1.0, np.inf)
        if kind == 2: m["smoothness"] = rng.choice([-3.0, 7.0, np.nan])
        if kind == 3: m["transmittance"], m["refraction_index"] = 1.0, -1.5
        if kind == 4: m["emission_strength"] = np.inf
        if kind == 5: m["metallic"] = np.nan
    box = R.box_triangles()
    mesh = S.blob_mesh(6, 5, seed=int(rng.randint(100)), smooth=bool(rng.randint(2)))  # 48 triangles
    extra = np.zeros(6, R.TRIANGLE)
    for k in range(6):  # hand-made triangles, some degenerate
        p = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
        if hostile and k % 3 == 0: p[2] = p[1]                      # zero area
        if hostile and k % 3 == 1: p[2] = p[0] + (p[1] - p[0]) * 0.5  # collinear
        extra[k] = R.flat_triangle(rng.normal(size=3), p[0], p[1], p[2])
    tris = R.concat(R.TRIANGLE, box, mesh, extra)
    shapes = []
    for _ in range(rng.randint(1, 10)):
        mat = int(rng.randint(n_mats))
        if hostile and rng.rand() < 0.1: mat = -1
        kind = rng.randint(4)
        if kind == 0:
            r = rng.uniform(0.1, 1.5)
            if hostile and rng.rand() < 0.2: r = rng.choice([0.0, -0.7, 1e-20, 1e20])
            shapes.append(R.sphere(mat, rng.uniform(-3, 3, 3), r))
        elif kind == 1:
            n = rng.normal(size=3) * rng.choice([1.0, 1e-3, 50.0])
            if hostile and rng.rand() < 0.2: n = np.zeros(3)
            shapes.append(R.plane(mat, rng.uniform(-3, 3, 3), n))
        elif kind == 2:
            first, cnt = [(0, 12), (12, len(mesh)), (12 + len(mesh), 6), (0, 0)][rng.randint(4)]
            tr = R.mat_mul(R.translate(rng.uniform(-2, 2, 3)), R.mat_mul(R.euler_yxz(*rng.uniform(-3, 3, 2)), R.scale_matrix(rng.uniform(0.2, 1.5, 3))))
            s = R.model(mat, tris, first, cnt, tr)
            if hostile and rng.rand() < 0.2:  # bounds that do not match the triangles (the UI's Box::model does that too)
                s["bounding_min"] -= rng.uniform(0, 2, 3).astype(np.float32)
                s["bounding_max"] = s["bounding_min"] + rng.uniform(0, 1, 3).astype(np.float32)
            shapes.append(s)
        else:
            s = R.sphere(mat, rng.uniform(-3, 3, 3), 1.0)
            s["type"] = 7 if hostile else 0  # unknown type: ignored by the kernel (render.cl:301-366)
            shapes.append(s)
    arr = np.zeros(len(shapes), R.SHAPE)
    for i, s in enumerate(shapes):
        arr[i] = s
    cam = R.camera_matrix(rng.uniform(-1, 1, 3) + np.array([0, 0.5, 4]), rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4))
    if hostile and rng.rand() < 0.2:
        cam[:3, :3] *= np.float32(rng.choice([0.0, 3.0]))  # degenerate / scaled rotation part
    return arr, tris, mats, cam


def random_options(rng, shapes, cam, w, h):
    """the render and scene records as test_random_scenes_match_oracle draws them behind random_scene (same calls, same order)"""
    rd = R.render_data(w, h, int(rng.randint(1, 5)), int(rng.choice([1, 2, 5, 10])), fov_scale=float(rng.uniform(0.3, 2.0)),
                       camera_to_world=cam, time=int(rng.randint(1, 2**31)), show_normals=bool(rng.rand() < 0.1))
    sd = R.scene_data(len(shapes), sun_focus=float(rng.choice([25.0, 1.0, 32.0, 7.5, 0.0, 100.0])), sun_intensity=float(rng.uniform(0, 3)))
    return rd, sd


# ---- thresholds, by the definition --------------------------------------------------------------------------------------
TWO_M32 = F(2.0 ** -32)


def u_of_r(r):
    """what the kernel's random_float makes of the generator's output r: float32(uint32 r) * float32(2^-32). r: int or array."""
    return (np.asarray(r, np.uint64).astype(np.uint32).astype(F) * TWO_M32).astype(F)


_threshold_cache = {}


def threshold_by_definition(p):
    """T(p) = the number of r in [0, 2^32) with p > u(r), p a float32. u is non-decreasing in r, so the set is a prefix and T
    the first r with not (p > u(r)): found by bisection over the DEFINITION's u (numpy float32), never through the library."""
    p = F(p)
    key = p.tobytes()
    if key not in _threshold_cache:
        lo, hi = 0, 1 << 32
        with np.errstate(all="ignore"):
            while lo < hi:
                mid = (lo + hi) >> 1
                if p > u_of_r(mid):
                    lo = mid + 1
                else:
                    hi = mid
        _threshold_cache[key] = lo
    return _threshold_cache[key]


# ---- the restatement of csrc/srt_abi.hip scene_class() -----------------------------------------------------------------
CLASS_LAYOUTS = {  # (blocks as (type, count)) -> {no_spec: class}
    ((R.SHAPE_PLANE, 2), (R.SHAPE_PLANE, 1), (R.SHAPE_SPHERE, 4)): {True: PPS, False: PPS_SPECULAR},
    ((R.SHAPE_SPHERE, 4),) * 3: {True: SSS},
    ((R.SHAPE_PLANE, 2),) * 3: {True: PPP},
}


def shape_blocks(shapes):
    """[(type, first shape, count)]: shapes of known type, in array order, in blocks of at most 4 spheres, 2 planes or 2 models;
    a new block on a type change, a gap in the indices (an unknown type in between) or a full block"""
    blocks = []
    for i, s in enumerate(shapes):
        ty = int(s["type"])
        if ty not in (R.SHAPE_SPHERE, R.SHAPE_PLANE, R.SHAPE_MODEL):
            continue
        cap = 4 if ty == R.SHAPE_SPHERE else 2
        if not blocks or blocks[-1][0] != ty or blocks[-1][1] + blocks[-1][2] != i or blocks[-1][2] == cap:
            blocks.append([ty, i, 0])
        blocks[-1][2] += 1
    return [tuple(b) for b in blocks]


def is_plain(c):
    c = F(c)
    return bool(np.isfinite(c) and not (c == 0 and np.signbit(c)))


def material_flags(mats):
    """-> (unit: every probability of every material has a threshold below 2^32; no_spec: every specular threshold is 0 and
    every colour component is finite and not -0)"""
    unit, spec0, plain = True, True, True
    for m in mats:
        for k in ("metallic", "specular", "transmittance"):
            if threshold_by_definition(m[k]) >> 32:
                unit = False
        if threshold_by_definition(m["specular"]) != 0:
            spec0 = False
        if not all(is_plain(c) for c in m["color"]):
            plain = False
    return unit, unit and spec0 and plain


def scene_lds_bytes(n_shapes, n_materials, n_groups=1):
    """device_types.h srt_scene_lds_bytes for a scene without models: 32 B per shape, 64 B per material, 16 + 192 B per block
    group; 0 = does not fit 4608 B"""
    b = n_shapes * 32 + n_materials * 64 + n_groups * (16 + 192)
    return b if b <= 4608 else 0


def expected_class(shapes, mats, rd, textured=False, count_tris=False):
    """the scene class the library must choose for a dispatch of rd over (shapes, mats)"""
    blocks = shape_blocks(shapes)
    if any(b[0] == R.SHAPE_MODEL for b in blocks):
        return GENERAL
    if not 1 <= len(blocks) <= 3:  # one group is at most three blocks
        return GENERAL
    nxt = 0
    for _, first, count in blocks:  # the blocks cover shapes 0 .. n - 1 with none left out
        if first != nxt:
            return GENERAL
        nxt += count
    if nxt != len(shapes):
        return GENERAL
    if any(int(s["material"]) < 0 for s in shapes):
        return GENERAL
    if scene_lds_bytes(len(shapes), len(mats)) == 0:
        return GENERAL
    unit, no_spec = material_flags(mats)
    if not unit:
        return GENERAL
    if int(rd["num_bounces"]) <= 0 or int(rd["show_normals"]) or textured or count_tris:
        return GENERAL
    return CLASS_LAYOUTS.get(tuple((ty, n) for ty, _, n in blocks), {}).get(no_spec, GENERAL)


# ---- draws shared by the lanes -------------------------------------------------------------------------------------------
DENORMAL = float(np.finfo(F).smallest_subnormal)
HOSTILE_P = [0.0, -0.0, -0.2, -np.inf, np.nan, 2.0 ** -33, 2.0 ** -32, DENORMAL, 0.5, 1.0 - 2.0 ** -24, 1.0]  # every one has a threshold below 2^32
HOSTILE_P_ZERO = [0.0, -0.0, -0.2, -np.inf, np.nan]  # ... of exactly 0: a "specular" that is never drawn
ABOVE_ONE = [float(np.nextafter(F(1), F(2))), 1.5, np.inf]  # no 32-bit threshold
HOSTILE_RADII = [0.0, -0.7, 1e-20, 1e20, 2.0 ** -41, 2.0 ** 41, np.nan]  # (2^-40 .. 2^40 is where the host keeps 1 / radius: inv_w)
HOSTILE_COLOURS = [(np.nan, 1.0, np.inf), (-0.0, 0.5, 0.25), (0.3, -np.inf, 0.9), (0.2, 0.4, -0.0)]


def pick(rng, values):
    return values[int(rng.randint(len(values)))]


def lane_materials(rng, n, specular):
    """n materials; specular False: every specular probability is 0 and every colour plain"""
    mats = np.zeros(n, R.MATERIAL)
    for i in range(n):
        mats[i] = R.material(rng.uniform(0, 1, 3), smoothness=rng.uniform(0, 1), metallic=rng.choice([0, 0, 1, rng.uniform()]),
                             specular=rng.choice([0, 0, rng.uniform(0.05, 1)]) if specular else 0.0,
                             transmittance=rng.choice([0, 0, 1, rng.uniform()]),
                             refraction_index=rng.choice([1.0, 1.5, 1.33, rng.uniform(0.5, 2.5)]),
                             emission=rng.uniform(0, 1, 3), emission_strength=rng.choice([0, 0, rng.uniform(0, 5)]))
    return mats


def hostile_material_edit(rng, m, specular):
    """one hostile value in material m that leaves every threshold below 2^32 (and, specular False, the specular one 0 and the
    colour plain)"""
    kind = int(rng.randint(7 if specular else 6))
    if kind == 0: m[pick(rng, ["metallic", "transmittance"])] = pick(rng, HOSTILE_P)
    if kind == 1: m["specular"] = pick(rng, HOSTILE_P if specular else HOSTILE_P_ZERO)
    if kind == 2: m["refraction_index"] = pick(rng, [0.0, -1.5])
    if kind == 3: m["smoothness"] = pick(rng, [-3.0, 7.0, np.nan])
    if kind == 4: m["emission_strength"] = np.inf
    if kind == 5: m["transmittance"], m["refraction_index"] = 1.0, pick(rng, [0.0, -1.5, 1.5])
    if kind == 6: m["color"] = pick(rng, HOSTILE_COLOURS)


def lane_sphere(rng, mat, hostile_rate):
    r = rng.uniform(0.1, 1.5)
    if rng.rand() < hostile_rate: r = pick(rng, HOSTILE_RADII)
    return R.sphere(mat, rng.uniform(-3, 3, 3), r)


def lane_plane(rng, mat, hostile_rate):
    n = rng.normal(size=3) * rng.choice([1.0, 1e-3, 50.0])
    if rng.rand() < hostile_rate: n = pick(rng, [np.zeros(3), n * 1e20, n * 1e-30])
    return R.plane(mat, rng.uniform(-3, 3, 3), n)


def stack(items, dtype):
    a = np.zeros(len(items), dtype)
    for i, it in enumerate(items):
        a[i] = it
    return a


def lane_camera(rng, shapes, hostile):
    """the fuzz's camera; one time in five inside a sphere of the scene or behind one of its planes"""
    pos = rng.uniform(-1, 1, 3) + np.array([0, 0.5, 4])
    if len(shapes) and rng.rand() < 0.2:
        s = shapes[int(rng.randint(len(shapes)))]
        with np.errstate(all="ignore"):
            if s["type"] == R.SHAPE_SPHERE and 0.05 < abs(float(s["sphere_radius"])) < 10:
                pos = s["sphere_position"].astype(np.float64) + rng.uniform(-0.4, 0.4, 3) * abs(float(s["sphere_radius"]))
            elif s["type"] == R.SHAPE_PLANE:
                n = s["plane_normal"].astype(np.float64)
                ln = np.sqrt((n * n).sum())
                if np.isfinite(ln) and ln > 1e-20:
                    pos = s["plane_position"].astype(np.float64) - n / ln * rng.uniform(0.1, 2.0) + rng.uniform(-1, 1, 3) * 0.2
    cam = R.camera_matrix(pos, rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4))
    if hostile and rng.rand() < 0.08:
        cam[:3, :3] *= np.float32(rng.choice([0.0, 3.0, 3.0]))  # zeroed (every ray the same: a blank frame) / scaled rotation part
    return cam


def lane_options(rng, shapes, cam, w, h):
    """spp 1..4, bounces of {1, 2, 5, 10}, fov, time, sun; no show_normals"""
    rd = R.render_data(w, h, int(rng.randint(1, 5)), int(rng.choice([1, 2, 5, 10])), fov_scale=float(rng.uniform(0.3, 2.0)),
                       camera_to_world=cam, time=int(rng.randint(1, 2**31)))
    d = rng.normal(size=3)
    d = d / np.sqrt((d * d).sum())
    sd = R.scene_data(len(shapes), sun_focus=float(rng.choice([25.0, 1.0, 32.0, 7.5, 0.0, 100.0])), sun_intensity=float(rng.uniform(0, 3)),
                      sun_direction=d.astype(F) if rng.rand() < 0.5 else None)
    return rd, sd


NO_TRIS = np.zeros(0, R.TRIANGLE)
CLASS_COUNTS = {PPS: (3, 4), PPS_SPECULAR: (3, 4), SSS: (0, 12), PPP: (6, 0)}  # planes, then spheres


def class_scene(rng, cls, hostile, w=FRAME[0], h=FRAME[1]):
    """a scene of class cls: its layout in array order, everything else random"""
    specular = cls == PPS_SPECULAR
    n_planes, n_spheres = CLASS_COUNTS[cls]
    n_mats = int(rng.randint(1, 8))
    mats = lane_materials(rng, n_mats, specular)
    if specular:  # at least one material whose specular threshold is not 0 or whose colour is not plain
        m = mats[int(rng.randint(n_mats))]
        if hostile and rng.rand() < 0.5:
            m["color"] = pick(rng, HOSTILE_COLOURS)
        else:
            m["specular"] = rng.uniform(0.05, 1.0) if not hostile else pick(rng, [2.0 ** -33, 2.0 ** -32, DENORMAL, 0.5, 1.0 - 2.0 ** -24, 1.0])
    if hostile:
        hostile_material_edit(rng, mats[int(rng.randint(n_mats))], specular)  # at least one, then each with one chance in three
        for i in range(n_mats):
            if rng.rand() < 1 / 3:
                hostile_material_edit(rng, mats[i], specular)
    if specular:  # (a later edit may have undone the first: the scene must stay specular)
        unit, no_spec = material_flags(mats)
        if no_spec:
            mats[0]["specular"] = 0.5
    # hostile shapes per scene: about one (a radius of 1e20 or 2^41 alone makes every pixel NaN; tests/test_fuzz_lanes.py holds the
    # share of such scenes below a quarter)
    rate = 0.0 if not hostile else (0.05 if cls == SSS else 0.12)
    items = [lane_plane(rng, int(rng.randint(n_mats)), rate) for _ in range(n_planes)]
    items += [lane_sphere(rng, int(rng.randint(n_mats)), rate) for _ in range(n_spheres)]
    shapes = stack(items, R.SHAPE)
    if cls == SSS and rng.rand() < 0.75:  # twelve small spheres leave most of the frame to the sky: one of them encloses the others
        k = int(rng.randint(n_spheres))
        shapes["sphere_position"][k] = rng.uniform(-1, 1, 3)
        shapes["sphere_radius"][k] = rng.uniform(6, 10) * (1 if not hostile else pick(rng, [1, 1, -1]))
    cam = lane_camera(rng, shapes, hostile)
    rd, sd = lane_options(rng, shapes, cam, w, h)
    return shapes, NO_TRIS, mats, cam, rd, sd


def class_lane(cls):
    def lane(rng, hostile, it):
        return (*class_scene(rng, cls, hostile), (cls, False), {})
    return lane


# ---- near misses ------------------------------------------------------------------------------------------------------------
NEAR_MISS_KINDS = ["no_material", "unknown_type", "spheres_first", "count", "probability_above_1", "colour_not_plain",
                   "specular_spheres", "too_many_materials", "show_normals", "no_bounces"]


def near_miss_lane(rng, hostile, it):
    """a class scene and ONE edit; expected = what the edit must do to the class"""
    kind = NEAR_MISS_KINDS[it % len(NEAR_MISS_KINDS)]
    base = {"spheres_first": [PPS, PPS_SPECULAR], "count": [SSS, PPP], "colour_not_plain": [PPS, SSS, PPP],
            "specular_spheres": [SSS, PPS]}.get(kind, [PPS, PPS_SPECULAR, SSS, PPP])
    turn = it // len(NEAR_MISS_KINDS)  # the variants of an edit come in turn, so that a short run has them all
    count_edit = [(SSS, "11"), (SSS, "13"), (SSS, "12+plane"), (PPP, "5"), (PPP, "7")][turn % 5]
    cls = count_edit[0] if kind == "count" else pick(rng, base)
    shapes, tris, mats, cam, rd, sd = class_scene(rng, cls, hostile)
    want = GENERAL
    what = kind
    if kind == "no_material":
        shapes["material"][int(rng.randint(len(shapes)))] = -1
    elif kind == "unknown_type":
        where = ["front", "middle", "end"][turn % 3]
        at = {"front": 0, "middle": len(shapes) // 2, "end": len(shapes)}[where]
        s = R.sphere(int(rng.randint(len(mats))), rng.uniform(-3, 3, 3), 1.0)
        s["type"] = pick(rng, [7, 3, -1])
        shapes = stack(list(shapes[:at]) + [s] + list(shapes[at:]), R.SHAPE)
        what = f"{kind}/{where}"
    elif kind == "spheres_first":
        shapes = stack(list(shapes[3:]) + list(shapes[:3]), R.SHAPE)
    elif kind == "count":
        edit = count_edit[1]
        if edit in ("11", "5"): shapes = shapes[:int(edit)].copy()
        if edit == "13": shapes = stack(list(shapes) + [lane_sphere(rng, 0, 0.0)], R.SHAPE)
        if edit in ("12+plane", "7"): shapes = stack(list(shapes) + [lane_plane(rng, 0, 0.0)], R.SHAPE)
        what = f"{kind}/{edit}"
    elif kind == "probability_above_1":
        mats[int(rng.randint(len(mats)))][pick(rng, ["metallic", "specular", "transmittance"])] = pick(rng, ABOVE_ONE)
    elif kind == "colour_not_plain":
        mats[int(rng.randint(len(mats)))]["color"] = pick(rng, HOSTILE_COLOURS)
        want = PPS_SPECULAR if cls == PPS else GENERAL
    elif kind == "specular_spheres":
        mats[int(rng.randint(len(mats)))]["specular"] = pick(rng, [2.0 ** -33, 0.5, 1.0])
        want = PPS_SPECULAR if cls == PPS else GENERAL
    elif kind == "too_many_materials":
        mats = R.concat(R.MATERIAL, mats, np.zeros(PAD_MATERIALS, R.MATERIAL))
    elif kind == "show_normals":
        rd["show_normals"] = 1
    elif kind == "no_bounces":
        rd["num_bounces"] = pick(rng, [0, 0, -1])
    sd["num_shapes"] = len(shapes)
    return shapes, tris, mats, cam, rd, sd, (want, False), {"edit": kind, "what": what, "base": cls}


# ---- the product's general kernels ---------------------------------------------------------------------------------------------
def shapes_only_scene(rng, hostile):
    """8..40 spheres and planes in random order: several block groups, no models"""
    mats = lane_materials(rng, int(rng.randint(1, 8)), True)
    if hostile:
        m = mats[int(rng.randint(len(mats)))]
        if rng.rand() < 0.3:
            m[pick(rng, ["metallic", "specular", "transmittance"])] = pick(rng, ABOVE_ONE + [2.0, -1.0])  # the float compares
        else:
            hostile_material_edit(rng, m, True)
    items = []
    for _ in range(int(rng.randint(8, 41))):
        mat = int(rng.randint(len(mats)))
        if hostile and rng.rand() < 0.05: mat = -1
        s = lane_sphere(rng, mat, 0.05 if hostile else 0.0) if rng.rand() < 0.6 else lane_plane(rng, mat, 0.1 if hostile else 0.0)
        if hostile and rng.rand() < 0.05: s["type"] = 7
        items.append(s)
    shapes = stack(items, R.SHAPE)
    return shapes, NO_TRIS, mats, lane_camera(rng, shapes, hostile)


def general_lane(kind):
    accel = ACCEL_BVH if kind.startswith("bvh") else ACCEL_NONE

    def lane(rng, hostile, it):
        if kind == "shapes_only":
            shapes, tris, mats, cam = shapes_only_scene(rng, hostile)
        else:
            shapes, tris, mats, cam = random_scene(rng, hostile)
            if rng.rand() < 0.95:  # random_scene leaves most frames mostly sky: a sphere around scene and camera, so that paths meet
                back = R.sphere(int(rng.randint(len(mats))), rng.uniform(-1, 1, 3), rng.uniform(9, 14))
                at = int(rng.randint(len(shapes) + 1))  # (somewhere in the array: the blocks change with it)
                shapes = stack(list(shapes[:at]) + [back] + list(shapes[at:]), R.SHAPE)
        if kind.endswith("_pad"):
            mats = R.concat(R.MATERIAL, mats, np.zeros(PAD_MATERIALS, R.MATERIAL))
        rd, sd = random_options(rng, shapes, cam, *FRAME)
        return shapes, tris, mats, cam, rd, sd, (expected_class(shapes, mats, rd), False), {"accel": accel}
    return lane


# ---- the textured twins ----------------------------------------------------------------------------------------------------
def constant_textures(rng, mats, tris, hostile):
    """every material (the first 64: SRT_MAX_TEXTURES) bound NEAREST to a 1x1 or 3x2 image whose texels all equal its colour
    -- NaN, inf and -0 included --, random UV scales, random mesh UVs on half the scenes. A NaN scale is not a binding the
    library accepts (include/srt_abi.h: a scale that is not finite is SRT_ERR_INVALID): `rejected` holds the bindings with
    it, which srt_update_scene must refuse, `bindings` the same with a finite scale in its place. NaN COORDINATES reach the
    sampler through NaN UVs and through hits at non-finite positions."""
    n_tex = min(len(mats), MAX_TEXTURES)
    images = []
    for i in range(n_tex):
        img = np.ones((2, 3, 4) if rng.rand() < 0.5 else (1, 1, 4), F)
        img[..., :3] = np.asarray(mats[i]["color"], F)
        images.append(img)
    bindings = np.zeros(len(mats), R.MATERIAL_TEXTURE)
    rejected = None
    for i in range(len(mats)):
        su, sv = (float(x) for x in rng.uniform(-4, 4, 2))
        if hostile and rng.rand() < 0.3:
            su = pick(rng, [1e30, -3e38, 0.0, np.nan])
        if hostile and rng.rand() < 0.3:
            sv = pick(rng, [1e30, -3e38, 0.0, np.nan])
        bindings[i] = R.material_texture(i if i < n_tex else -1, NEAREST, su, sv)
    if np.isnan(bindings["scale_u"]).any() or np.isnan(bindings["scale_v"]).any():
        rejected = bindings.copy()
        for k in ("scale_u", "scale_v"):
            bindings[k] = np.where(np.isnan(bindings[k]), F(2.5), bindings[k])
    uvs = None
    if len(tris) and rng.rand() < 0.5:
        uvs = rng.uniform(-2, 3, (len(tris), 3, 2)).astype(F)
        if hostile:
            bad = rng.rand(*uvs.shape) < 0.03
            uvs[bad] = rng.choice([np.inf, -np.inf, np.nan], size=int(bad.sum())).astype(F)
    return {"images": images, "bindings": bindings, "rejected": rejected, "uvs": uvs}


def varying_textures(rng, mats, tris, hostile):
    """constant_textures' bindings, scales, UVs and refused NaN scale, but the images are 1x1 to 5x4 with random finite texels
    that are not negative, and the filters are random: the expectation is the TEXTURED oracle's canvas."""
    tex = constant_textures(rng, mats, tris, hostile)
    images = []
    for _ in tex["images"]:
        img = np.ones((int(rng.randint(1, 5)), int(rng.randint(1, 6)), 4), F)
        img[..., :3] = rng.uniform(0.0, 1.5, img.shape[:2] + (3,)).astype(F)
        images.append(img)
    for b in (tex["bindings"], tex["rejected"]):
        if b is not None:
            b["filter"] = np.where(rng.rand(len(mats)) < 0.5, LINEAR, NEAREST)
    return dict(tex, images=images, varying=True)


def textured_lane(kind, varying=False):
    def lane(rng, hostile, it):
        if kind == "class":
            base = class_lane((PPS, PPS_SPECULAR, SSS, PPP)[it % 4])
        elif kind == "shapes_only":
            base = general_lane(kind)
        else:  # scan / bvh: plain and with the padding materials in turn
            base = general_lane(kind + ("_pad" if it % 2 else ""))
        shapes, tris, mats, cam, rd, sd, _, extra = base(rng, hostile, it)
        extra = dict(extra, textures=(varying_textures if varying else constant_textures)(rng, mats, tris, hostile))
        return shapes, tris, mats, cam, rd, sd, (GENERAL, not rd["show_normals"]), extra
    return lane


LANES = {"class1": class_lane(PPS), "class2": class_lane(PPS_SPECULAR), "class3": class_lane(SSS), "class4": class_lane(PPP),
         "near_miss": near_miss_lane,
         "scan": general_lane("scan"), "bvh": general_lane("bvh"), "scan_pad": general_lane("scan_pad"), "bvh_pad": general_lane("bvh_pad"),
         "shapes_only": general_lane("shapes_only"),
         "tex_scan": textured_lane("scan"), "tex_bvh": textured_lane("bvh"), "tex_shapes_only": textured_lane("shapes_only"),
         "tex_class": textured_lane("class"),
         "texvar_scan": textured_lane("scan", True), "texvar_bvh": textured_lane("bvh", True),
         "texvar_shapes_only": textured_lane("shapes_only", True), "texvar_class": textured_lane("class", True)}
CLASS_LANES = {"class1": PPS, "class2": PPS_SPECULAR, "class3": SSS, "class4": PPP}
# iterations per case = SRT_FUZZ_ITERS (default 300) * share: 50 per class lane, 60 near misses (6 of each edit), 40 per general and
# per tex_* lane, 20 per texvar_* lane -- 1,400 scenes over both flavours (tests/test_gpu_fuzz_dispatch.py has the measured cost).
# 20: a texvar lane's deterministic branches (plain / padded in turn, the four classes in turn, a budget every third scene) come
# round in 12 scenes, and its random ones (both filters, a 1x1 and a 4x5 image, a refused NaN scale when hostile) have all been
# drawn by scene 19 at the latest over the eight cases (texvar_shapes_only benign; the others by scene 12), which
# tests/test_fuzz_lanes.py asserts at the count in use; 20 is the next share of the base count.
LANE_SHARE = {name: (1, 5) if name == "near_miss" else (1, 6) if name in CLASS_LANES else (1, 15) if name.startswith("texvar_") else (2, 15)
              for name in LANES}


def lane_iterations(name, base=300):
    num, den = LANE_SHARE[name]
    return max(1, base * num // den)


def lane_seed(name, hostile, seed=20250):
    return seed + 2 * sorted(LANES).index(name) + int(hostile)


# ---- the runner: one Tracer per case, every scene through update_scene, all checks -------------------------------------------------
COUNTERS = ("paths", "rays", "sky", "nan_pixels")


def bits_equal(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def differing_pixels(got, want):
    return int((~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).any(axis=-1).sum())


def run_lane(T, oracle, sky, name, hostile, iterations, seed=20250, nthreads=4, progress=None, report=None):
    """`iterations` scenes of lane `name` on one Tracer (T: the simple_raytracer_amd.tracer module). For every scene: the class
    and the textured flag the library reports equal the lane's intention AND the restatement; the canvas is the oracle's bit
    for bit; paths, rays, sky, nan_pixels are the oracle's; the watchdog did not fire. On a third of the scenes a radiance
    budget forces two or three sample batches. report: a list that receives (class, plane form, textured) of every dispatch as the
    library reports them. -> (failures [(lane, iteration, what, differing pixels, differing counters)],
    classes reported [int], edits {kind: count})"""
    lane = LANES[name]
    rng = np.random.RandomState(lane_seed(name, hostile, seed))
    w, h = FRAME
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.count_triangles(False)
    failures, classes, edits = [], [], {}
    try:
        for it in range(iterations):
            shapes, tris, mats, cam, rd, sd, expected, extra = lane(rng, hostile, it)
            problems = []
            t.set_acceleration(extra.get("accel", ACCEL_NONE))
            tex = extra.get("textures")
            t.options, t.scene_data = rd, sd
            if tex is not None:
                t.set_textures(tex["images"])
                t.set_triangle_uvs(tex["uvs"])
                if tex["rejected"] is not None:  # a NaN scale: refused, and the handle goes on with what it is given next
                    t.set_material_textures(tex["rejected"])
                    try:
                        t.update_scene(shapes, tris, mats)
                        problems.append("a NaN texture scale was accepted")
                    except T.SrtError:
                        pass
                t.set_material_textures(tex["bindings"])
            spp = int(rd["num_samples"])
            t.set_radiance_budget(w * h * 12 * max(1, spp // 2) if it % 3 == 2 else 0)  # 12 bytes per pixel and sample: batches of spp // 2
            t.update_scene(shapes, tris, mats)
            t.clear_canvas()
            t.reset_counters()
            t.trace()
            got, c = t.read_canvas(), t.counters()
            reported = (t.last_trace_class(), t.last_trace_textured())
            classes.append(reported[0])
            if report is not None:
                report.append((reported[0], t.last_trace_plane_form(), reported[1]))
            restated = (expected_class(shapes, mats, rd, textured=expected[1]), expected[1])
            if not (reported == tuple(expected) == restated):
                problems.append(f"class / textured: library {reported}, lane {tuple(expected)}, restatement {restated}")
            with np.errstate(all="ignore"):
                if tex is not None and tex.get("varying"):
                    table = texture_cases.oracle_table((shapes, tris, mats), tex["images"], tex["bindings"], tex["uvs"])
                    want, oc = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table, counters=True, nthreads=nthreads)
                else:
                    want, oc = oracle.render(rd, sd, shapes, tris, mats, sky, counters=True, nthreads=nthreads)
            bad = differing_pixels(got, want)
            ctr = {k: (c[k], oc[k]) for k in COUNTERS if c[k] != oc[k]}
            if c["watchdog"] != 0:
                ctr["watchdog"] = (c["watchdog"], 0)
            if not bits_equal(got, want) or ctr or problems:
                failures.append((name, it, "; ".join(problems + [extra.get("what", "")]).strip("; "), bad, ctr))
            if "edit" in extra:
                edits[extra["edit"]] = edits.get(extra["edit"], 0) + 1
            if progress:
                progress(it, failures)
    finally:
        t.close()
    return failures, classes, edits
