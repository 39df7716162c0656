"""What the GPU tests share: the library fixture T (every GPU test module), and for the denoiser's tests
(tests/test_gpu_denoise*.py) a configured Tracer, the scenes, the cameras of a moving sequence and the tonemap curve. A
plain module, not a test module: the tests import from it, and pytest finds the fixture T in the namespace of the test
module that imports it."""
import numpy as np
import pytest

import cases as C
import denoise_ref as D
from simple_raytracer_amd import records as R, scenes as S


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def scene(name):
    """spheres, meshes or mixed (any other name) -> shapes, tris, mats"""
    if name == "spheres":
        return S.sphere_scene()
    if name == "meshes":
        return S.mesh_scene()
    return S.mixed_test_scene()


def guide_scene(name):
    """the guide-buffer tests' scenes (SCENES) -> shapes, tris, mats, camera"""
    cam = S.default_camera()
    if name == "spheres":
        return (*S.sphere_scene(), cam)
    if name == "mixed":
        return (*S.mixed_test_scene(), R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15))
    if name == "glass":  # the camera inside a glass sphere: back faces
        return (*C.glass_scene(), cam)
    if name == "boxes":  # rotated, non-uniformly scaled box instances
        return (*C.box_instances_scene(), R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15))
    if name == "mesh_smooth":
        return (*S.mesh_scene(2, 10, 11, smooth=True), cam)
    if name == "mesh_flat":
        return (*S.mesh_scene(1, 8, 7, smooth=False), cam)
    if name == "empty":
        return (*C.empty_scene(), cam)
    if name == "no_material":  # shapes without a material: their hits are misses
        shapes, tris, mats = S.mixed_test_scene()
        shapes = shapes.copy()
        shapes["material"][[1, 4]] = -1
        return shapes, tris, mats, R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15)
    raise ValueError(name)


SCENES = [("spheres", 0), ("mixed", 0), ("mixed", 1), ("glass", 0), ("boxes", 0), ("mesh_smooth", 0), ("mesh_smooth", 1),
          ("mesh_flat", 0), ("mesh_flat", 1), ("empty", 0), ("no_material", 0), ("no_material", 1)]


def make(T, sky, scn, w, h, spp=2, accel=0, time=777, cam=None, show_normals=False, denoise=None, temporal=None, motion=False):
    """A Tracer over scn (a name of scene() or (shapes, tris, mats)), cleared, camera cam (None: the default camera), with the
    denoiser (set_denoise(**denoise)), temporal reprojection and object motion on when given. t.scene = the arrays."""
    shapes, tris, mats = scene(scn) if isinstance(scn, str) else scn
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera() if cam is None else cam, time=time, show_normals=show_normals)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    if denoise is not None:
        t.set_denoise(**denoise)
    if temporal is not None:
        t.set_denoise_temporal(**temporal)
    if motion:
        t.set_denoise_object_motion(True)
    t.scene = (shapes, tris, mats)
    return t


def cam_at(k, kind):
    """camera of frame k of a path: still (None: the default camera), small moves in x, y and z (move), or yaw / pitch
    steps from the default camera"""
    if kind is None:
        return S.default_camera()
    if kind == "move":
        return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)
    if kind == "yaw":
        return R.camera_matrix((0.0, 0.5, 5.0), 0.011 * k, 0.0)
    return R.camera_matrix((0.0, 0.5, 5.0), 0.004 * k, 0.009 * k)


def tone(x):
    """the tonemapped value the resolve turns into a byte: sqrt(aces(x)), in [0, 1]"""
    return np.sqrt(D._aces1(np.asarray(x, np.float32))).astype(np.float64)
