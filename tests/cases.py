"""Named parity cases shared by the golden generator, the CPU tests and the GPU tests.

Each case -> dict(shapes, tris, mats, rd, sd, frames) where frames is a list of
`time` seeds rendered into ONE canvas without clearing (progressive accumulation,
/root/reference/src/main.cpp:277-290)."""
import numpy as np

from simple_raytracer_amd import records as R, scenes as S


def _case(scene, w, h, spp, nb=10, frames=(12345,), cam=None, fov=1.0, **kw):
    shapes, tris, mats = scene
    cam = S.default_camera() if cam is None else cam
    rd = R.render_data(w, h, spp, nb, fov_scale=fov, camera_to_world=cam, time=frames[0], **kw)
    sd = R.scene_data(len(shapes))
    return dict(shapes=shapes, tris=tris, mats=mats, rd=rd, sd=sd, frames=list(frames))


def glass_scene():
    """Glass-heavy: nested refractive spheres and a camera INSIDE a glass sphere."""
    mats = np.zeros(4, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    mats[1] = R.material((0.95, 1.0, 0.95), smoothness=1.0, transmittance=1.0, refraction_index=1.5)
    mats[2] = R.material((1.0, 0.9, 0.9), smoothness=0.6, transmittance=0.8, refraction_index=1.33, specular=0.1)
    mats[3] = R.material((1, 1, 1), emission=(1, 0.9, 0.7), emission_strength=3.0)
    shapes = np.zeros(6, R.SHAPE)
    shapes[0] = R.plane(0, (0, -1, 0), (0, 1, 0))
    shapes[1] = R.sphere(1, (0, 0.5, 5.0), 1.2)      # camera sits inside this one
    shapes[2] = R.sphere(1, (0.0, 0.2, 1.0), 1.2)
    shapes[3] = R.sphere(2, (0.0, 0.2, 1.0), 0.6)    # nested
    shapes[4] = R.sphere(2, (-2.2, 0.0, 0.5), 1.0)
    shapes[5] = R.sphere(3, (2.5, 2.0, 0.0), 0.5)
    return shapes, R.box_triangles(), mats


def box_instances_scene():
    """Box instances sharing the 12 box triangles (src/shape.cpp:76-89), including
    rotated and non-uniformly scaled copies made like the GUI's gizmo does."""
    mats = np.zeros(3, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.9))
    mats[1] = R.material((0.9, 0.4, 0.2), smoothness=0.3, specular=0.2)
    mats[2] = R.material((0.3, 0.5, 0.9), smoothness=0.9, metallic=0.8)
    tris = R.box_triangles()
    shapes = np.zeros(5, R.SHAPE)
    shapes[0] = R.plane(0, (0, -1, 0), (0, 1, 0))
    shapes[1] = R.box_model(1, 0, (-2.0, 0.0, -1.0))
    shapes[2] = R.box_model(2, 0, (1.5, 0.0, -2.0))
    shapes[3] = R.model(1, tris, 0, 12, R.mat_mul(R.translate((0.0, -0.3, 1.0)), R.mat_mul(R.euler_yxz(0.5, 0.4, 0.0), R.scale_matrix((0.4, 0.7, 0.4)))))
    shapes[4] = R.model(2, tris, 0, 12, R.mat_mul(R.translate((2.6, 1.2, 0.3)), R.mat_mul(R.euler_yxz(-1.0, 0.2, 0.0), R.scale_matrix((0.3, 1.1, 0.6)))))
    return shapes, tris, mats


def empty_scene():
    """What the app starts with: no shapes, one default material, 12 box triangles
    (src/main.cpp:95-102)."""
    mats = np.zeros(1, R.MATERIAL)
    mats[0] = R.material()
    return np.zeros(0, R.SHAPE), R.box_triangles(), mats


def build_cases():
    cam_tilt = R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15)
    return {
        "spheres": _case(S.sphere_scene(), 64, 64, 8),
        "spheres_accum": _case(S.sphere_scene(), 48, 40, 3, frames=(12345, 987654321, 77)),
        "normals": _case(S.mixed_test_scene(), 64, 48, 2, show_normals=True),
        "glass": _case(glass_scene(), 64, 48, 6),
        "boxes": _case(box_instances_scene(), 64, 48, 4, cam=cam_tilt),
        "mixed": _case(S.mixed_test_scene(), 64, 48, 4, cam=cam_tilt, fov=0.8),
        "mesh_smooth": _case(S.mesh_scene(2, 10, 11, smooth=True), 48, 40, 3),
        "mesh_flat": _case(S.mesh_scene(1, 8, 7, smooth=False), 48, 40, 3),
        "empty": _case(empty_scene(), 32, 24, 2),
        "one_bounce": _case(S.sphere_scene(), 40, 30, 4, nb=1),
        "ragged": _case(S.sphere_scene(), 37, 29, 3, nb=4),
        "even_time": _case(S.sphere_scene(), 32, 24, 4, frames=(4096,)),  # time*5304 loses low bits
    }


def render_case(render_fn, case, sky):
    """Accumulate all frames of a case with `render_fn(rd, canvas) -> canvas`."""
    canvas = None
    for tm in case["frames"]:
        rd = case["rd"].copy()
        rd["time"] = np.uint32(tm & 0xFFFFFFFF)
        canvas = render_fn(rd, canvas)
    return canvas


# ---- the renders of tests/test_oracle_vs_ref.py and tests/test_oracle_statistics.py; tests/golden/ref_checks.npz holds the
# ---- reference build's outputs for them, so both tests also run where oracle/_ref cannot be built
AVERAGE_STEPS = (1, 3)
STATS_SPP = 256
STATS_SEEDS = (12345, 777)  # the compared render's seed, and the other seed of the noise floor


def ref_check_frames():
    """name -> (scene, width, height, spp, render_data keywords) of the frames the port and the reference build render alike."""
    out = {"sphere_slab": (S.sphere_scene(), 256, 32, 16, {}),  # a 32-row slab of config[0]
           "mesh": (S.mesh_scene(2), 80, 45, 2, {}),
           "average_input": (S.sphere_scene(), 64, 48, 4, {})}
    for tm in (1, 2**31, 0xFFFFFFFF, 1700000000123 & 0xFFFFFFFF):
        out[f"seed_{tm}"] = (S.mixed_test_scene(), 40, 30, 2, {"time": tm})
    return out


def render_frame(o, frame, sky):
    """One frame of ref_check_frames() by the checker `o`: x, y, z only (the 4th lane of an OpenCL float3 is unspecified and
    the reference build leaves register garbage in it)."""
    (shapes, tris, mats), w, h, spp, kw = frame
    rd = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), **kw)
    sd = R.scene_data(len(shapes))
    return o.render(rd, sd, shapes, tris, mats, sky, nthreads=4)[..., :3]


def average_input(canvas_xyz):
    """The canvas test_average_bytes resolves: a rendered frame plus NaN poisoning and out-of-range values."""
    a = np.concatenate([canvas_xyz, np.zeros_like(canvas_xyz[..., :1])], axis=-1)
    a[0, 0, :3] = np.nan  # must resolve to byte 0, not crash
    a[0, 1, :3] = (1e9, 0.0, -1.0)
    return a


def stats_render(o, case, sky, time_seed):
    """A golden case rendered by `o` at STATS_SPP samples with another seed: x, y, z (float32) of the canvas."""
    rd = case["rd"].copy()
    rd["num_samples"] = STATS_SPP
    rd["time"] = np.uint32(time_seed)
    return o.render(rd, case["sd"], case["shapes"], case["tris"], case["mats"], sky, nthreads=8)[..., :3]


def big_models_between_shapes(seed):
    """Big models (>= 128 triangles: the array scan suspends the rays that enter their boxes, csrc/trace_body.inc) with
    spheres, planes, boxes and a second instance of the same mesh BEHIND them in the shape array, overlapping boxes,
    glass and mirror materials: a suspended ray has to come back with its closest hit so far and see every later shape."""
    rng = np.random.RandomState(seed)
    mats = np.zeros(6, R.MATERIAL)
    mats[0] = R.material((0.8, 0.8, 0.8))
    mats[1] = R.material((0.5, 0.9, 0.6), smoothness=1.0, transmittance=0.9, refraction_index=1.4)
    mats[2] = R.material((0.9, 0.7, 0.3), smoothness=0.8, metallic=0.7)
    mats[3] = R.material((0.3, 0.4, 0.9), specular=0.3, smoothness=0.9)
    mats[4] = R.material((1, 1, 1), emission=(1.0, 0.8, 0.5), emission_strength=2.0)
    mats[5] = R.material((0.9, 0.2, 0.2))
    box = R.box_triangles()
    mesh_a = S.blob_mesh(14, 9, seed=seed, smooth=True)        # 2 * 14 * 8 = 224+ triangles: big
    mesh_b = S.blob_mesh(10, 9, seed=seed + 1, smooth=False)   # big as well, flat shaded
    tris = R.concat(R.TRIANGLE, box, mesh_a, mesh_b)
    ia, ib = 12, 12 + len(mesh_a)
    assert len(mesh_a) >= 128 and len(mesh_b) >= 128
    xf = lambda p, yaw, s: R.mat_mul(R.translate(p), R.mat_mul(R.euler_yxz(yaw, 0.2, 0.0), R.scale_matrix(s)))
    shapes = [
        R.sphere(2, (-2.4, 0.2, -1.5), 0.7),
        R.model(1, tris, ia, len(mesh_a), xf((-0.6, 0.1, -1.0), 0.5, (1.0, 1.0, 1.0))),   # big, glass
        R.plane(0, (0, -1.1, 0), (0, 1, 0)),                                               # after a big model
        R.sphere(4, (0.3, 2.2, -1.0), 0.5),
        R.model(2, tris, ib, len(mesh_b), xf((1.2, 0.0, -1.8), -0.8, (0.9, 1.2, 0.9))),   # big, overlaps the first one's box
        R.model(3, tris, 0, 12, xf((0.2, -0.6, 0.4), 0.3, (0.3, 0.3, 0.3))),               # small (box) after the big ones
        R.model(5, tris, ia, len(mesh_a), xf((0.4, 0.3, -2.6), 2.0, (0.8, 0.8, 0.8))),    # second instance of mesh a
        R.sphere(3, (2.3, -0.3, -0.4), 0.6),
    ]
    a = np.zeros(len(shapes), R.SHAPE)
    for i, s in enumerate(shapes):
        a[i] = s
    return a, tris, mats
