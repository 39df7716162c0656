"""The queries' one staging allocation (csrc/query_stage.h; the host forms of csrc/ray_query.hip and csrc/occlusion.hip): calls
of every kind on ONE handle, their counts growing and shrinking, each against the same call on a fresh handle of the same
scene, bit for bit. The regions of one call alias those of another (hits and segments, picked points and the masks) and the
offsets move with n, so a call that read what an earlier one left behind, or wrote past its own regions, would show here."""
import numpy as np
import pytest

import occlusion_cases as O
from gpu_harness import T  # noqa: F401 (the fixture)
from ray_query_cases import frame_rd, scene
from simple_raytracer_amd import records as R, scenes as S
from test_gpu_ray_query import handle

pytestmark = pytest.mark.gpu
F = np.float32


def rays_of(n, seed):
    """n rays between ordinary points, directions of any length, four of them hostile (for the invalid mask)"""
    s = O.random_segments(n, seed)
    r = R.rays(s["from"], s["to"] - s["from"])
    r["direction"][0] = 0.0
    r["tmax"][n // 2] = np.nan
    r["origin"][n - 1, 1] = np.inf
    r["tmax"][1] = F(2.5)
    return r


def calls():
    """(name, the call on a handle -> its results as a tuple of arrays), in the order that moves every offset both ways"""
    rd = frame_rd(S.default_camera())
    a, b, c = rays_of(257, 21), rays_of(65, 22), rays_of(65, 23)
    s, u = O.random_segments(257, 24), O.random_segments(65, 25)
    return [("cast_rays 257", lambda t: (t.cast_rays(a),)),
            ("occluded_rays 65", lambda t: t.occluded_rays(b, with_invalid=True)),
            ("pick 1", lambda t: (t.pick([[3.5, 1.5]], options=rd),)),
            ("occluded_segments 257", lambda t: t.occluded_segments(s, with_invalid=True)),
            ("segment_rays 65", lambda t: (t.segment_rays(u),)),
            ("cast_rays 65", lambda t: (t.cast_rays(c),))]


@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "scan"), ("mesh_smooth", "sah")])
def test_interleaved_calls_equal_fresh_handles(name, accel, T):
    assert name == "spheres" or (scene(name)[0]["type"] == R.SHAPE_MODEL).sum() == 2
    one = handle(T, name, accel)
    seen = {}
    for what, call in calls():
        got = call(one)
        fresh = handle(T, name, accel)
        want = call(fresh)
        fresh.close()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, accel, what)
        seen[what] = got
    one.close()
    # and the calls are not vacuous: hits and misses, occluded and visible, refused rays, finite rays of segments
    hit = (seen["cast_rays 257"][0]["flags"] & R.HIT_HIT) != 0
    assert hit.any() and not hit.all() and ((seen["cast_rays 65"][0]["flags"] & R.HIT_INVALID_RAY) != 0).sum() == 3
    occ, inv = seen["occluded_rays 65"]
    assert occ.any() and not occ.all() and inv.sum() == 3 and not (occ & inv).any()
    occ, inv = seen["occluded_segments 257"]
    assert occ.any() and not occ.all() and not inv.any()
    assert np.isfinite(seen["segment_rays 65"][0]["tmax"]).all() and len(seen["pick 1"][0]) == 1
