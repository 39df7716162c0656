"""What the texture tests share (tests/test_gpu_texture.py, tests/test_gpu_texture_paths.py, tests/test_oracle_textures.py):
the white first-hit scenes with their textures and bindings, the numpy route to the texel at a primary hit
(tests/texture_ref.py at the oracle's primary hits), the table the textured oracle takes, and the deep-path cases whose
canvases the GPU tests hold to the textured oracle. A plain module, not a test module."""
import numpy as np

import cases
import texture_ref as TR
from simple_raytracer_amd import records as R, scenes as S

F = np.float32


def bind_all(n_materials, texture_of, filt=TR.NEAREST, scale=(1.0, 1.0)):
    b = np.zeros(n_materials, R.MATERIAL_TEXTURE)
    for i in range(n_materials):
        b[i] = R.material_texture(texture_of(i), filt, *scale)
    return b


def constant_textures(mats, side):
    out = []
    for m in mats:
        img = np.ones((side, side, 4), F)
        img[..., :3] = np.asarray(m["color"], F).reshape(-1)[:3]
        out.append(img)
    return out


# ---- the texel at the first hit ---------------------------------------------------------------------------------------------
def white_scene():
    """three spheres and two planes (one tilted), every shape its own white diffuse material"""
    mats = np.array([R.material(color=(1, 1, 1)) for _ in range(5)], R.MATERIAL)
    shapes = np.array([R.sphere(0, (-1.6, 0.4, -1.0), 0.9), R.sphere(1, (0.3, 0.1, 0.5), 0.6), R.sphere(2, (1.7, 0.8, -2.0), 1.3),
                       R.plane(3, (0.0, -0.5, 0.0), (0.0, 1.0, 0.0)), R.plane(4, (0.0, 0.0, -6.0), (0.3, 0.2, 1.0))], R.SHAPE)
    return shapes, np.zeros(0, R.TRIANGLE), mats


def white_mesh_scene():
    """two rotated, non-uniformly scaled box instances over triangle ranges of their own and a floor plane, every shape its
    own white diffuse material"""
    mats = np.array([R.material(color=(1, 1, 1)) for _ in range(3)], R.MATERIAL)
    tris = R.concat(R.TRIANGLE, R.box_triangles(), R.box_triangles())
    m0 = R.mat_mul(R.mat_mul(R.translate((-1.5, 0.7, 0.8)), R.euler_yxz(0.6, 0.35, 0.2)), R.scale_matrix((1.4, 1.0, 0.8)))
    m1 = R.mat_mul(R.mat_mul(R.translate((1.5, 0.5, 0.2)), R.euler_yxz(-0.4, 0.2, -0.3)), R.scale_matrix((0.9, 1.5, 1.2)))
    shapes = np.array([R.model(0, tris, 0, 12, m0), R.plane(1, (0.0, -0.8, 0.0), (0.0, 1.0, 0.0)), R.model(2, tris, 12, 12, m1)], R.SHAPE)
    return shapes, tris, mats


def mesh_uvs():
    return np.random.default_rng(17).uniform(-1.5, 2.5, (24, 3, 2)).astype(F)


def mesh_bindings(filt):
    b = np.zeros(3, R.MATERIAL_TEXTURE)
    b[0] = R.material_texture(0, filt, 3.0, 2.0)
    b[1] = R.material_texture(2, filt, 0.5, 0.25)
    b[2] = R.material_texture(1, filt, -2.0, 1.5)
    return b


# (scene, bindings, accel, with UVs): spheres and planes; a mesh with UVs and without, array scan and BVH
FIRST_HIT_CASES = [("shapes", 0, False), ("mesh", 0, True), ("mesh", 0, False), ("mesh", 1, True), ("mesh", 1, False)]


def first_hit_case(kind, filt, with_uvs):
    if kind == "shapes":
        return white_scene(), white_bindings(filt), None
    return white_mesh_scene(), mesh_bindings(filt), (mesh_uvs() if with_uvs else None)


TEXTURES = [TR.checker(8, 8), TR.gradient(16, 8), TR.checker(5, 3, (0.8, 0.3, 0.2), (0.2, 0.7, 0.9))]


def white_bindings(filt):
    b = np.zeros(5, R.MATERIAL_TEXTURE)
    b[0] = R.material_texture(0, filt, 4.0, 2.0)
    b[1] = R.material_texture(1, filt, 1.0, 1.0)
    b[2] = R.material_texture(2, filt, 1e30, 5.0)  # u * 1e30 * fW >= 2^30 (but at u = 0): texel (0, 0)
    b[3] = R.material_texture(0, filt, 0.5, 0.5)
    b[4] = R.material_texture(1, filt, 0.25, -3e38)  # v * -3e38 * fH overflows to an infinity where |v| > 0.15: texel (0, 0)
    return b


def model_hit_uv(oracle, shapes, tris, s, cam, d, t, X, uvs):
    """UV of primary hits on model s: the triangle by the oracle's intersect_triangle in array order (first of equal t) on the
    world-space vertices of its matrix_by_vector, the weights by its barycentric_weights at X (they come as w2, w0, w1)."""
    ti, n = int(shapes["triangle_index"][s]), int(shapes["num_triangles"][s])
    P = [[oracle.matrix_by_vector(shapes["transform"][s], np.append(tris["v"]["pos"][ti + j][k], F(1)))[:3] for k in range(3)] for j in range(n)]
    u, v = np.zeros(len(d), F), np.zeros(len(d), F)
    for i in range(len(d)):
        best, bt = -1, F(np.inf)
        for j in range(n):
            hit, tt = oracle.intersect_triangle(*P[j], cam, d[i])
            if hit and tt < bt:
                best, bt = j, tt
        assert best >= 0 and bt == t[i], (s, i, bt, t[i])
        w = oracle.barycentric_weights(*P[best], X[i])
        uu, vv = TR.model_uv(w[1], w[2], w[0], None if uvs is None else uvs[ti + best])
        u[i], v[i] = uu[0], vv[0]
    return u, v


def first_hit_texels(oracle, rd, sd, scn, bindings, ids, smp, uvs=None):
    """texture_ref at the oracle's primary hits -> (n, 3) texels ((1, 1, 1) where nothing is hit), hit mask"""
    shapes, tris, mats = scn
    ph = oracle.primary_hits(rd, sd, shapes, tris, mats, ids, smp)
    cam = np.asarray(rd["camera_to_world"], F).reshape(4, 4)[3, :3]
    d, t = ph["dir"].astype(F), ph["t"].astype(F)
    with np.errstate(all="ignore"):
        X = (cam[None, :] + d * t[:, None]).astype(F)  # org + dir * tmin
    out = np.ones((len(ids), 3), F)
    hit = ph["material"] >= 0
    for s in range(len(shapes)):  # every shape has its own material
        sel = hit & (ph["material"] == shapes["material"][s])
        if not sel.any():
            continue
        b = bindings[shapes["material"][s]]
        if shapes["type"][s] == R.SHAPE_SPHERE:
            u, v = TR.sphere_uv(X[sel], shapes["sphere_position"][s], shapes["sphere_radius"][s])
        elif shapes["type"][s] == R.SHAPE_MODEL:
            u, v = model_hit_uv(oracle, shapes, tris, s, cam, d[sel], t[sel], X[sel], uvs)
        else:
            Tn, Bn = TR.plane_frame(shapes["plane_normal"][s])
            u, v = TR.plane_uv(X[sel], shapes["plane_position"][s], Tn, Bn)
        out[sel] = TR.sample(TEXTURES[b["texture"]], b["filter"], u, v, b["scale_u"], b["scale_v"])
    return out, hit


# ---- the table of the textured oracle ----------------------------------------------------------------------------------------
def oracle_table(scn, images, bindings, uvs=None, first_hit_only=False):
    """oracle_py.TextureTable for a scene: the plane frames come from texture_ref.plane_frame (float64, rounded), which
    tests/test_texture_host.py holds bit-equal to the library's srt_plane_frame_host."""
    from oracle import oracle_py
    shapes, tris, mats = scn
    frames = [TR.plane_frame(shapes["plane_normal"][s]) if shapes["type"][s] == R.SHAPE_PLANE else None for s in range(len(shapes))]
    return oracle_py.TextureTable(images, bindings, len(mats), len(shapes), len(tris), frames, uvs, first_hit_only)


# ---- deep paths: the scenes whose whole canvas is held to the textured oracle ------------------------------------------------------
def noise_texture(w=7, h=5, seed=5):
    """seeded noise in [0.05, 0.95], every texel distinct in every channel"""
    img = np.ones((h, w, 4), F)
    img[..., :3] = np.random.default_rng(seed).permutation(3 * w * h).reshape(h, w, 3).astype(F) / F(3 * w * h) * F(0.9) + F(0.05)
    assert len(np.unique(img[..., 0])) == w * h
    return img


PATH_TEXTURES = TEXTURES + [noise_texture()]  # 8x8 checker, 16x8 gradient, 5x3 two-colour, 7x5 noise
PATH_SCALES = [(4.0, 2.0), (-1.5, 0.75), (2.5, -3.25), (0.5, 0.5), (0.3, -0.7), (1.0, 1.0), (-2.0, 1.5), (3.0, 0.37)]


def coat_texture():
    """the specular coat's: an 8x8 checker with two texels for which mix(t, 1, 1) = fma(1 - t, 1, t) is NOT 1.0f (it is for every
    t in [0, 1.5]: 1 - t rounds by at most half an ulp of 1): 2^24 + 2 gives 2, 5e8 gives 0. Finite and not negative, so in
    contract; they make the texel's bits count at a specular bounce, where a colour "is ignored"."""
    img = TR.checker(8, 8, (0.85, 0.8, 0.7), (0.3, 0.5, 0.4))
    img[2, 3, 0] = F(16777218.0)
    img[5, 6, 1] = F(5e8)
    return img


def path_bindings(n_materials, filt, first=0):
    b = np.zeros(n_materials, R.MATERIAL_TEXTURE)
    for i in range(n_materials):
        b[i] = R.material_texture((first + i) % len(PATH_TEXTURES), filt, *PATH_SCALES[i % len(PATH_SCALES)])
    return b


def material_scene(no_specular=False, pad_materials=0):
    """The white scene's geometry with a mirror, a glass sphere (paths hit its inside), a rough metal, a specular coat on the
    floor, a diffuse wall, a small emitter and a plane whose normal is zero (no frame: it keeps its colour; nothing hits
    it). no_specular: every specular probability 0 -- with these plain colours the kernels take the `mask * colour`
    shortcut. pad_materials more materials: the scene records leave the LDS copy."""
    mats = np.array([R.material(color=(0.9, 0.9, 0.9), metallic=1.0, smoothness=1.0),
                     R.material(color=(0.9, 0.95, 0.9), smoothness=1.0, transmittance=0.9, refraction_index=1.4),
                     R.material(color=(0.8, 0.6, 0.3), metallic=0.8, smoothness=0.4),
                     R.material(color=(0.7, 0.7, 0.7), specular=0.0 if no_specular else 0.5, smoothness=0.9),
                     R.material(color=(0.9, 0.9, 0.9)),
                     R.material(color=(1.0, 0.9, 0.8), emission=(1.0, 0.8, 0.5), emission_strength=2.0),
                     R.material(color=(0.2, 0.4, 0.6))], R.MATERIAL)
    if pad_materials:
        mats = R.concat(R.MATERIAL, mats, np.zeros(pad_materials, R.MATERIAL))
    shapes = np.array([R.sphere(0, (-1.6, 0.4, -1.0), 0.9), R.sphere(1, (0.3, 0.1, 0.5), 0.6), R.sphere(2, (1.7, 0.8, -2.0), 1.3),
                       R.plane(3, (0.0, -0.5, 0.0), (0.0, 1.0, 0.0)), R.plane(4, (0.0, 0.0, -6.0), (0.3, 0.2, 1.0)),
                       R.sphere(5, (0.2, 1.9, -0.8), 0.35), R.plane(6, (0.0, -3.0, 0.0), (0.0, 0.0, 0.0))], R.SHAPE)
    return shapes, np.zeros(0, R.TRIANGLE), mats


MATERIAL_TEXTURES = PATH_TEXTURES + [coat_texture()]


def material_bindings(n_materials, filt):
    b = path_bindings(7, filt)
    b[3] = R.material_texture(4, filt, 0.5, -0.25)  # the floor's coat: coat_texture, one repeat per 2 x 4 units
    if n_materials > 7:
        b = R.concat(R.MATERIAL_TEXTURE, b, np.array([R.material_texture()] * (n_materials - 7), R.MATERIAL_TEXTURE))
    return b


def mesh_path_scene():
    """white_mesh_scene's rotated, non-uniformly scaled boxes, now a diffuse box, a glass box (bounce rays reach its triangles
    from inside), a mirror floor (and from outside, from below the horizon of the camera) and a third instance that shares
    the first one's triangle range under another material and texture."""
    mats = np.array([R.material(color=(0.9, 0.9, 0.9)),
                     R.material(color=(0.9, 0.9, 0.9), metallic=1.0, smoothness=0.95),
                     R.material(color=(0.9, 0.95, 0.9), smoothness=1.0, transmittance=0.9, refraction_index=1.4),
                     R.material(color=(0.6, 0.8, 0.7), specular=0.3, smoothness=0.8)], R.MATERIAL)
    tris = R.concat(R.TRIANGLE, R.box_triangles(), R.box_triangles())
    m0 = R.mat_mul(R.mat_mul(R.translate((-1.5, 0.7, 0.8)), R.euler_yxz(0.6, 0.35, 0.2)), R.scale_matrix((1.4, 1.0, 0.8)))
    m1 = R.mat_mul(R.mat_mul(R.translate((1.5, 0.5, 0.2)), R.euler_yxz(-0.4, 0.2, -0.3)), R.scale_matrix((0.9, 1.5, 1.2)))
    m2 = R.mat_mul(R.mat_mul(R.translate((0.0, 0.2, -0.8)), R.euler_yxz(1.1, -0.3, 0.4)), R.scale_matrix((1.1, 0.8, 1.3)))
    shapes = np.array([R.model(0, tris, 0, 12, m0), R.plane(1, (0.0, -0.8, 0.0), (0.0, 1.0, 0.0)), R.model(2, tris, 12, 12, m1),
                       R.model(3, tris, 0, 12, m2)], R.SHAPE)
    return shapes, tris, mats


def big_model_scene():
    """tests/test_gpu_large_scene.py's big models (>= 128 triangles: suspended scans), glass and mirror among them"""
    return cases.big_models_between_shapes(11)


def big_uvs(n):
    return np.random.default_rng(23).uniform(-1.0, 2.0, (n, 3, 2)).astype(F)


def path_case(name, filt=TR.LINEAR, with_uvs=True, w=37, h=29):
    """A deep-path case by name -> dict(scn, cam, images, bindings, uvs, w, h, spp, bounces, time). Names: material,
    material_pad (80 padding materials), material_nospec, material_nospec_pad, mesh, big."""
    cam = S.default_camera()
    if name.startswith("material"):
        scn = material_scene(no_specular="nospec" in name, pad_materials=80 if name.endswith("pad") else 0)
        return dict(scn=scn, cam=cam, images=MATERIAL_TEXTURES, bindings=material_bindings(len(scn[2]), filt), uvs=None, w=w, h=h, spp=4, bounces=10, time=4242)
    if name == "mesh":
        scn = mesh_path_scene()
        cam = R.camera_matrix((0.0, 0.1, 2.6), 0.0, -0.1)  # low and close: the ragged 33x7 frame too sees the floor and the boxes
        return dict(scn=scn, cam=cam, images=PATH_TEXTURES, bindings=path_bindings(4, filt, first=1), uvs=mesh_uvs() if with_uvs else None,
                    w=w, h=h, spp=4, bounces=10, time=4242)
    if name == "big":
        scn = big_model_scene()
        cam = R.camera_matrix((0.3, 0.6, 1.2), 0.0, -0.25)  # close to the models: a third of the paths meet a texture after their first hit
        return dict(scn=scn, cam=cam, images=PATH_TEXTURES, bindings=path_bindings(len(scn[2]), filt, first=2),
                    uvs=big_uvs(len(scn[1])) if with_uvs else None, w=64, h=40, spp=3, bounces=10, time=4253)
    raise ValueError(name)


PATH_CASE_NAMES = ["material", "material_pad", "material_nospec", "material_nospec_pad", "mesh", "big"]
FRAMES = [(37, 29), (33, 7)]  # (the big models render at their own 64x40)
# every view tests/test_gpu_texture_paths.py renders, filters apart: (name, with UVs, w, h). tests/test_oracle_textures.py asserts
# the coverage condition on each of them.
GPU_VIEWS = ([(n, True, w, h) for n in PATH_CASE_NAMES[:4] for w, h in FRAMES] + [("mesh", uv, w, h) for uv in (True, False) for w, h in FRAMES]
             + [("big", True, 64, 40), ("big", False, 64, 40)])


def case_render_data(case):
    rd = R.render_data(case["w"], case["h"], case["spp"], case["bounces"], camera_to_world=case["cam"], time=case["time"])
    return rd, R.scene_data(len(case["scn"][0]))


def oracle_path_canvas(oracle, sky, case, rd=None, sd=None, counters=False, first_hit_only=False):
    """The textured oracle's canvas of a case (rd / sd: the tracer's own records where a GPU test has them)."""
    if rd is None:
        rd, sd = case_render_data(case)
    shapes, tris, mats = case["scn"]
    table = oracle_table(case["scn"], case["images"], case["bindings"], case["uvs"], first_hit_only)
    return oracle.render_textured(rd, sd, shapes, tris, mats, sky, table, counters=counters)
