"""What the ray-query tests share (tests/test_ray_query_host.py, tests/test_gpu_ray_query.py): the scenes, the two cameras of
each, the oracle's primary hits of their 8x4 frames (computed once per scene and camera, never changed) and the image points of
a sample's primary ray. A plain module, not a test module."""
import functools

import numpy as np

import cases as C
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
FW, FH, NS, TIME = 8, 4, 2, 777

# every scene with the default camera and with one moved and turned well away from it, both chosen (with the oracle, on the
# CPU) so that the 64 rays of each scene's frames give hits and misses: the check below asserts it
CAMERAS = {
    "spheres": (S.default_camera(), R.camera_matrix((4.0, 1.5, -5.0), -3.0, -0.1)),
    "boxes": (S.default_camera(), R.camera_matrix((-5.0, 4.0, -3.0), -2.3, -0.45)),
    "mesh_smooth": (S.default_camera(), R.camera_matrix((-5.0, 4.0, -3.0), -2.3, -0.45)),
    "mesh_flat": (S.default_camera(), R.camera_matrix((-5.0, 4.0, -3.0), -2.3, -0.45)),
}
ACCELS = {"spheres": ("scan",), "boxes": ("scan", "sah"), "mesh_smooth": ("scan", "sah", "median"), "mesh_flat": ("scan", "sah", "median")}


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "spheres":
        return S.sphere_scene()
    if name == "boxes":
        return C.box_instances_scene()
    if name == "mesh_smooth":
        return S.mesh_scene(2, 10, 11, smooth=True)
    return S.mesh_scene(1, 8, 7, smooth=False)


def frame_rd(cam, w=FW, h=FH, ns=NS, time=TIME, fov=1.0):
    return R.render_data(w, h, ns, 10, fov_scale=fov, camera_to_world=cam, time=time)


_oracle_cache = {}


def primary(oracle, name, k, shapes=None):
    """the oracle's primary hits of every (pixel, sample) of camera k's 8x4 frame: ids, samples, dict(dir, t, normal, material)"""
    key = (name, k) if shapes is None else None
    if key in _oracle_cache:
        return _oracle_cache[key]
    sh, tr, ma = scene(name)
    sh = sh if shapes is None else shapes
    ids, sm = np.repeat(np.arange(FW * FH), NS), np.tile(np.arange(NS), FW * FH)
    ph = o_hits(oracle, frame_rd(CAMERAS[name][k]), sh, tr, ma, ids, sm)
    if key is not None:
        _oracle_cache[key] = (ids, sm, ph)
    return ids, sm, ph


_close = {}


def close_mesh(oracle):
    """the smooth-mesh scene from close by and with a narrow field of view, so that the 8x4 frame shows both meshes, the plane and
    the sky: rd, ids, samples and the oracle's primary hits of every (pixel, sample)"""
    if not _close:
        sh, tr, ma = scene("mesh_smooth")
        rd = frame_rd(R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0), fov=0.5)
        ids, sm = np.repeat(np.arange(FW * FH), NS), np.tile(np.arange(NS), FW * FH)
        _close["v"] = (rd, ids, sm, o_hits(oracle, rd, sh, tr, ma, ids, sm))
    return _close["v"]


def sphere_closeup(oracle, shapes=None):
    """the sphere scene through a narrow field of view, so that the 8x4 frame puts several rays on each of the spheres in the
    middle of the view (shape 4 among them): rd, ids, samples and the oracle's primary hits; shapes: an edited shape array"""
    if shapes is None and "s" in _close:
        return _close["s"]
    sh, tr, ma = scene("spheres")
    rd = frame_rd(S.default_camera(), fov=0.25)
    ids, sm = np.repeat(np.arange(FW * FH), NS), np.tile(np.arange(NS), FW * FH)
    v = (rd, ids, sm, o_hits(oracle, rd, sh if shapes is None else shapes, tr, ma, ids, sm))
    if shapes is None:
        _close["s"] = v
    return v


def o_hits(oracle, rd, sh, tr, ma, ids, sm):
    with np.errstate(all="ignore"):
        return oracle.primary_hits(rd, R.scene_data(len(sh)), sh, tr, ma, ids, sm)


def jitter_xy(oracle, rd, ids, samples):
    """xy of the primary rays of (pixel, sample) pairs: float32(px) + r0, float32(py) + r1 with the sample's two random floats"""
    w, ns, time = int(rd["width"]), int(rd["num_samples"]), int(rd["time"])
    xy = np.zeros((len(ids), 2), F)
    for k, (i, s) in enumerate(zip(ids, samples)):
        seed = ((int(s) + int(i) * ns) * time * 5304) & 0xFFFFFFFF
        (r0, r1), _ = oracle.random_floats(seed, 2)
        xy[k] = F(int(i) % w) + r0, F(int(i) // w) + r1
    return xy
