"""What the X-ray area selection tests share (tests/test_area_through_host.py, tests/test_gpu_area_through.py): the scenes of the
existing builders, the frame and camera of each -- chosen with the oracle, on the CPU, so that every frame SEES THROUGH: some pixel
has at least three candidates and some shape is met on more pixels than it is visible on (the host test asserts it) -- and the
acceleration modes each is run under. A plain module, not a test module."""
import functools

import numpy as np

import cases as C
from ray_query_cases import scene
from simple_raytracer_amd import records as R, scenes as S

# the sphere scene at 130x6: rectangle widths 1, 63, 64, 65 and 130 and heights 1, 3, 4, 5 and 6 cross wave and workgroup edges
# (aspect_ratio is set by hand: the frame is a strip, the view is not)
SCENES = {
    "spheres": dict(w=130, h=6, cam=S.default_camera(), fov=0.3, aspect=4.0, accels=("scan",)),
    "boxes": dict(w=24, h=16, cam=R.camera_matrix((1.0, 1.2, 4.5), 0.25, -0.15), fov=1.0, aspect=None, accels=("scan", "sah", "median")),
    "mesh_smooth": dict(w=16, h=10, cam=R.camera_matrix((0.0, 0.3, 2.0), 0.0, 0.0), fov=0.5, aspect=None, accels=("scan", "sah", "median", "refit")),
    "glass": dict(w=24, h=16, cam=S.default_camera(), fov=1.0, aspect=None, accels=("scan",)),  # the camera inside sphere 1
}


def arrays(name):
    return C.glass_scene() if name == "glass" else scene(name)


def frame_of(name, w=None, h=None):
    """the scene's render data; w, h: another frame under the same camera"""
    c = SCENES[name]
    given = w is not None
    w, h = (c["w"], c["h"]) if w is None else (w, h)
    return R.render_data(w, h, 1, 2, fov_scale=c["fov"], camera_to_world=c["cam"], time=777, aspect_ratio=None if given else c["aspect"])


@functools.lru_cache(maxsize=None)
def moved_mesh_scene():
    """the smooth-mesh scene with its first model moved: what a refitted hierarchy has to answer for"""
    sh, tr, ma = scene("mesh_smooth")
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    return moved, tr, ma
