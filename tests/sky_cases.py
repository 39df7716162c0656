"""Skies, cameras and frames that put the sky lookup (csrc/device_shading.h sample_sky under sky_box) on its edges: image sizes
of 1, odd and prime sizes, a wide image with an odd row stride, HDR texels, an alpha lane of NaN, texels that are not plain
numbers; cameras that straddle the seam at -x, look up and down the poles, and -- with fov_scale = 0 -- aim every pixel at
one exact direction. A plain module, not a test module: tests/test_sky_cases.py checks on the CPU that the set holds what it
claims (coverage counts, mutants of tests/sky_ref.py), tests/test_gpu_sky_edges.py feeds it to the device.

The frame of a case is one sample of an EMPTY scene with the sun's intensity at 0: the canvas is sky_box(camera direction) + 0,
and oracle_py.Oracle.primary_hits gives each pixel's direction."""
import numpy as np

import cases as C
from simple_raytracer_amd import records as R, scenes as S

F = np.float32
SIZES = [(1, 1), (1, 5), (7, 1), (3, 2), (5, 7), (31, 13), (4099, 3)]  # W x H; 4099 is prime: an odd row stride of 65584 bytes
FRAMES = [(32, 24), (37, 29)]  # 37 x 29 = 1073 pixels: a ragged last wave
DENORMAL = F(np.finfo(F).smallest_subnormal)


def hdr_sky(w, h):
    """(h, w, 4): every colour value of the image distinct, in [0, 4), exact in float32 -- value k of the w * h * 3 is
    ((k * 611953 + 7919) mod 2^20) / 2^18 (an odd multiplier permutes the residues; 4099 * 3 * 3 < 2^20) --, alpha 1."""
    assert w * h * 3 < 2 ** 20
    k = np.arange(w * h * 3, dtype=np.int64)
    img = np.ones((h, w, 4), F)
    img[..., :3] = (((k * 611953 + 7919) % 2 ** 20).astype(F) / F(2 ** 18)).reshape(h, w, 3)
    return img


def nan_alpha(img):
    out = img.copy()
    out[..., 3] = np.nan
    return out


# the specials sky: (column, row) -> value of all three channels. The numbers sit where the fixed cameras look (corners, the
# seam column, the texels around +x); +inf and NaN sit away from every one of those footprints, so that only frames of the
# moving cameras meet them.
SPECIAL_TEXELS = {(0, 0): F(-0.0), (4, 6): DENORMAL, (2, 3): F(-1.75), (0, 3): F(1e30), (1, 2): F(np.inf), (3, 5): F(np.nan)}


def specials_sky():
    img = hdr_sky(5, 7)
    for (i, j), value in SPECIAL_TEXELS.items():
        img[j, i, :3] = value
    return img


def skies():
    """name -> (H, W, 4) float32. FINITE names the skies whose colours are all plain HDR numbers."""
    out = {f"{w}x{h}": hdr_sky(w, h) for w, h in SIZES}
    out["5x7_nan_alpha"] = nan_alpha(out["5x7"])
    out["3x2_nan_alpha"] = nan_alpha(out["3x2"])
    out["specials"] = specials_sky()
    return out


FINITE = [f"{w}x{h}" for w, h in SIZES]


def fixed_camera(target, flip_z=False):
    """A camera for fov_scale = 0, whose pixels all look along `target`: dir = normalize(((c0 * +-0 + c1 * +-0) - c2) + origin *
    0) with c2 = -target. A component of target that is +0 comes out +0 in every pixel; one that is -0 comes out -0 only in the
    pixels where the other three terms are -0 too (the origin is negative for that; the quadrant left of and below the centre),
    +0 elsewhere: such a frame holds both."""
    m = R.identity4()
    m[2, :3] = -np.asarray(target, F)
    m[3, :3] = (-1.0, -1.0, -1.0)
    if flip_z:
        m[0, 2] = -0.0
    return m


def cameras():
    """name -> (camera_to_world, fov_scale). MOVING: every pixel its own direction; FIXED: fov_scale = 0."""
    out = {"default": (S.default_camera(), 1.0),
           "seam": (R.camera_matrix((0, 0, 0), np.pi / 2, 0.0), 1.0),  # looks along -x: u runs from 0 to 1 across the frame
           "up": (R.camera_matrix((0, 0, 0), 0.0, 1.5), 2.0),
           "down": (R.camera_matrix((0, 0, 0), 0.0, -1.5), 2.0),
           "yaw_pi": (R.camera_matrix((0, 0, 0), np.pi, 0.0), 1.0),
           # (a narrower view of each pole: every column of the smaller skies meets the clamped row)
           "up_zoom": (R.camera_matrix((0, 0, 0), 0.3, 1.5), 0.5),
           "down_zoom": (R.camera_matrix((0, 0, 0), 0.3, -1.5), 0.5)}
    for name, target in FIXED_TARGETS.items():
        out[name] = (fixed_camera(target, name in FLIP_Z), 0.0)
    return out


FIXED_TARGETS = {"at_+y": (0.0, 1.0, 0.0), "at_-y": (0.0, -1.0, 0.0),
                 "at_-x_z+0": (-1.0, 0.0, 0.0), "at_-x_z-0": (-1.0, 0.0, -0.0), "at_-x_z+1e-7": (-1.0, 0.0, 1e-7), "at_-x_z-1e-7": (-1.0, 0.0, -1e-7),
                 # the seam below and above the middle rows: with at_-x_z-0, every pair of rows of a 3-row image on both sides of the seam
                 # (y = -0.894, -0.447, +0.894 once normalised), which no moving camera's pixels hit on an image 4099 texels wide
                 "at_-x_y-2": (-1.0, -2.0, -0.0), "at_-x_y-0.5": (-1.0, -0.5, -0.0), "at_-x_y+2": (-1.0, 2.0, -0.0),
                 "at_+x": (1.0, 0.0, 0.0),
                 # the zero vector with zeros of both signs: (-0, -0, -0) in one quadrant (atan2pi(-0, -0) = -1: u = 0), +0 elsewhere
                 # (u = 0.5); at_zero_u1 has (-0, y, +0) there instead (atan2pi(+0, -0) = 1: u = 1)
                 "at_zero": (-0.0, -0.0, -0.0), "at_zero_u1": (-0.0, -0.0, -0.0), "at_nan": (np.nan, 0.0, 0.0)}
FLIP_Z = {"at_zero_u1"}  # cameras whose first column has z = -0: the z of a pixel is -0 where its x is +0 and the other way round
MOVING = ["default", "seam", "up", "down", "yaw_pi", "up_zoom", "down_zoom"]


def empty_scene():
    return C.empty_scene()


def render_data(cam, fov, w, h, spp=1, time=4711):
    return R.render_data(w, h, spp, 10, fov_scale=fov, camera_to_world=cam, time=time)


def scene_data(sun=False):
    """the sun off (intensity 0: the frame is the lookup alone) or on, with the library's default lobe (focus 25)"""
    return R.scene_data(0, sun_intensity=1.0 if sun else 0.0)


def directions(oracle, cam, fov, w, h):
    """(w * h, 3): the direction of sample 0 of every pixel, row-major"""
    shapes, tris, mats = empty_scene()
    ids = np.arange(w * h, dtype=np.int32)
    return oracle.primary_hits(render_data(cam, fov, w, h), scene_data(), shapes, tris, mats, ids, np.zeros_like(ids))["dir"].copy()


def oracle_frame(oracle, sky, cam, fov, w, h, spp=1, sun=False, canvas=None, counters=False):
    shapes, tris, mats = empty_scene()
    with np.errstate(all="ignore"):
        return oracle.render(render_data(cam, fov, w, h, spp), scene_data(sun), shapes, tris, mats, sky, canvas=canvas, counters=counters,
                             nthreads=4)


def random_directions(n=200, seed=20261):
    d = np.random.RandomState(seed).normal(size=(n, 3))
    return (d / np.sqrt((d * d).sum(axis=1))[:, None]).astype(F)


REF_CHECK_SKIES = ["3x2", "5x7", "specials"]


def ref_check_directions(oracle):
    """The directions tests/golden/ref_checks.npz "sky/*" holds the reference build's sky_box for: every distinct direction
    (bit patterns: the signs of the zeros count) of the fov_scale = 0 cameras' 32 x 24 frames, then 200 random unit vectors."""
    w, h = FRAMES[0]
    cams = cameras()
    fixed = np.concatenate([directions(oracle, *cams[name], w, h) for name in FIXED_TARGETS])
    fixed = np.unique(np.ascontiguousarray(fixed).view(np.uint32), axis=0).view(F)
    return np.concatenate([fixed, random_directions()]).astype(F)
