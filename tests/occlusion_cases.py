"""What the occlusion-query tests share (tests/test_occlusion_host.py, tests/test_gpu_occlusion.py): the hostile rays, the ray
sets of the early-exit cases, the segments of the sphere scene with their answers, and the float64 restatement of the segment
kernel with its error bound. A plain module, not a test module."""
import numpy as np

from simple_raytracer_amd import records as R, scenes as S

F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32: one correctly rounded operation is off by at most U relative


def words_of(bits):
    """bool[n] -> the uint64 words of the mask: ray q is bit q & 63 of word q >> 6, the tail bits 0"""
    b = np.zeros((len(bits) + 63) // 64 * 64, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


# ---- hostile rays (DESIGN.md 25's list) ------------------------------------------------------------------------------------------
def hostile_rays(origin, direction, unit):
    """12 rays along `direction` from `origin`, some of them spoilt -> (rays, indices of the spoilt ones)"""
    rays = R.rays(origin, np.tile(np.asarray(direction, F), (12, 1)))
    rays["origin"][0, 1] = np.nan
    rays["direction"][1, 2] = np.inf
    rays["direction"][2] = 0.0
    rays["tmax"][3] = np.nan
    rays["origin"][5, 0] = -np.inf
    rays["direction"][6, 0] = np.nan
    rays["origin"][9, 2] = np.inf
    rays["direction"][10, 1] = -np.inf
    bad = [0, 1, 2, 3, 5, 6, 9, 10]
    if not unit:
        rays["direction"][7] = (1e-30, 0.0, 0.0)  # its squared length underflows
        rays["direction"][8] = (1e30, 1e30, 0.0)  # ... overflows
        bad += [7, 8]
    return rays, sorted(bad)


# ---- early exit -------------------------------------------------------------------------------------------------------------------
EYE = np.asarray((0.0, 0.5, 5.0), F)


def fan(target, spread, n=64, seed=3):
    """n unit directions from EYE towards points within `spread` of `target`"""
    rng = np.random.default_rng(seed)
    pts = np.asarray(target, np.float64) + rng.uniform(-spread, spread, (n, 3))
    d = pts - EYE.astype(np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def rays_all_behind_the_first_run():
    """sphere scene: 64 rays down and forward, all of which end on the floor (shape 0, in the first block of the first run)"""
    return R.rays(EYE, fan((0.0, -1.0, 2.0), 1.0))


def rays_one_lane_left(lane=37):
    """... but for one lane, which looks up and back past every shape: the wave cannot leave before the last run, and that lane
    must stay visible"""
    r = rays_all_behind_the_first_run()
    r["direction"][lane] = np.asarray((0.0, 0.8, 0.6), F)
    return r


def rays_one_lane_for_a_later_run(lane=11):
    """... but for one lane that stops short of the planes and is occluded only by sphere 4, in the last run"""
    r = rays_all_behind_the_first_run()
    c = np.asarray((0.5, 0.8, -3.0), np.float64)
    d = c - EYE
    r["direction"][lane] = (d / np.linalg.norm(d)).astype(F)
    r["tmax"][lane] = F(np.linalg.norm(d))  # ends at the centre of the sphere, three units in front of the back wall
    return r


MESH_CENTRES = ((-1.3, 0.1, -1.0), (1.4, 0.0, -1.6))  # scenes.mesh_scene(2, ...): shapes 1 and 2, one block of two models


def rays_two_models():
    """mesh scene: even lanes end at the centre of the first model, odd lanes at the centre of the second (tmax = the distance
    to the centre, so the floor behind them does not count): the first model of the block occludes half of the wave"""
    dirs, tmax = np.zeros((64, 3), F), np.zeros(64, F)
    for m in (0, 1):
        pts = np.asarray(MESH_CENTRES[m], np.float64) + np.random.default_rng(5 + m).uniform(-0.15, 0.15, (32, 3))
        d = pts - EYE
        n = np.linalg.norm(d, axis=1, keepdims=True)
        dirs[m::2], tmax[m::2] = (d / n).astype(F), n[:, 0].astype(F)
    return R.rays(EYE, dirs, tmax)


# ---- segments on the sphere scene -------------------------------------------------------------------------------------------------
# sphere 4 of scenes.sphere_scene(): centre (0.5, 0.8, -3), radius 1; seen along -z from A its front surface is at z = -2
A = (0.5, 0.8, 5.0)
SEGMENTS = [  # (from, to, end_gap, answer)
    (A, (0.5, 0.8, -5.0), 0.0, "occluded"),               # through the centre
    ((3.0, 3.0, 5.0), (3.0, 3.0, -5.0), 0.0, "visible"),  # beside every sphere, above the floor, in front of the back wall
    (A, (0.5, 0.8, -1.9), 0.0, "visible"),                # ends 0.1 in front of the sphere
    (A, (0.5, 0.8, -2.1), 0.0, "occluded"),               # ... 0.1 behind its surface
    (A, (0.5, 0.8, -2.05), 0.0, "occluded"),              # ends 0.05 inside the sphere
    (A, (0.5, 0.8, -2.05), 0.1, "visible"),               # ... and stops 0.1 short of that
    (A, A, 0.0, "invalid"),
    (A, (0.5, 0.8, -5.0), -0.5, "invalid"),
    (A, (0.5, 0.8, -5.0), np.nan, "invalid"),
    (A, (0.5, 0.8, -5.0), np.inf, "invalid"),
    (A, (0.5, np.inf, -5.0), 0.0, "invalid"),
    ((np.nan, 0.8, 5.0), (0.5, 0.8, -5.0), 0.0, "invalid"),
]


def sphere_segments():
    s = R.segments([a for a, _, _, _ in SEGMENTS], [b for _, b, _, _ in SEGMENTS], [g for _, _, g, _ in SEGMENTS])
    return s, [w for _, _, _, w in SEGMENTS]


def random_segments(n=257, seed=11):
    """ordinary segments: ends within 8 units of the origin, at least half a unit apart, gaps up to a tenth of the length"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-8.0, 8.0, (n, 3)).astype(F)
    b = (a + rng.uniform(0.5, 6.0, (n, 1)) * fan((0, 0, 0), 4.0, n, seed + 1)).astype(F)
    gap = (rng.uniform(0.0, 0.1, n) * np.linalg.norm(b.astype(np.float64) - a, axis=1)).astype(F)
    gap[::7] = 0.0
    return R.segments(a, b, gap)


def segment_rays_f64(segs):
    """The segment kernel's formulas in float64 from the float32 inputs -> (direction, tmax, length), and the bounds on what
    float32 may differ by.

    With u = 2^-24 and every float32 operation correctly rounded (relative error <= u), first order in u:
      d = to - from            one rounding: each component is off by <= u |d_i|
      s = dot3(d, d)           fma(z, z, fma(y, y, x x)): three roundings of sums of non-negative terms, <= 3u, on top of the
                               squares of components that are off by u each, <= 2u: s is off by <= 5u relative
      r = rsqrt(s)             detmath's rsqrt is within 1.00 ulp of the true value, and an ulp is at most
                               2^-23 = 2u relative; the true 1 / sqrt moves by half of s's error, 2.5u: <= 4.5u
      dir_i = d_i r            one rounding, d_i's u and r's 4.5u: <= 6.5u |dir_i|
      L = dot3(d, dir)         every product d_i dir_i = d_i^2 r is non-negative, so relative errors do not grow in the sum:
                               u + 6.5u per product, one rounding for the product or the fma and at most two more for the
                               sums above it: <= 10.5u L
      tmax = L - end_gap       one rounding of the result: <= 10.5u L + u |tmax|
    The second-order terms are below 100 u^2 = 6e-6 u; 6.5 and 10.5 are rounded up to 7 and 11 to hold them.
    """
    a, b, gap = segs["from"].astype(np.float64), segs["to"].astype(np.float64), segs["end_gap"].astype(np.float64)
    d = b - a
    length = np.linalg.norm(d, axis=1)
    direction = d / length[:, None]
    tmax = length - gap
    return direction, tmax, 7 * U * np.abs(direction), 11 * U * length + U * np.abs(tmax)


def sphere_scene():
    return S.sphere_scene()
