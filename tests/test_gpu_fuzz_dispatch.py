"""GPU (MI355X): the differential fuzz over every trace kernel the library launches, as the product launches them
(count_triangles off): the four scene-class kernels, the general instantiations without triangle counting -- array scan and
BVH, scene records in LDS and in global memory, sphere / plane scenes of several block groups --, and their textured twins.
The lanes are tests/fuzz_scenes.py's (benign and hostile); tests/test_fuzz_lanes.py checks, without a GPU, that they hold
what they claim. One Tracer per case, every scene through update_scene (so the class lanes also change classes on a live
handle), a ragged 23x17 frame, a radiance budget that forces two or three sample batches on every third scene.

For every scene: last_trace_class() and last_trace_textured() equal the lane's intention and the Python restatement of the
predicate (no lane can pass by falling back); the canvas is the oracle's bit for bit (NaN == NaN); paths, rays, sky and
nan_pixels are the oracle's; the watchdog did not fire.

Iterations per case: SRT_FUZZ_ITERS (default 300) times the lane's share (fuzz_scenes.LANE_SHARE): 50 per class lane, 60
near misses, 40 per general and tex_* lane, 20 per texvar_* lane (random texels and filters against the TEXTURED oracle; the
smallest share that visits every branch of their generator: fuzz_scenes.LANE_SHARE); 1,400 scenes over the 36 cases.
Measured on one MI355X box (the oracle on 4 threads is the cost): RUNTIME below."""
import os

import pytest

import fuzz_scenes as FS

pytestmark = pytest.mark.gpu

# Measured on an MI355X box, pytest's call durations summed: tests/test_gpu_fuzz.py (600 scenes) plus the fuzz of
# tests/test_gpu_bvh.py (150 scenes) 1.11 s (3.3 s with start-up); this module at its defaults, before the texvar_* lanes
# (1,240 scenes), 1.79 s (4.0 s): 1.6x. With them (1,400 scenes, measured in a later session) 1.96 s (4.30 s with start-up), of which
# the eight texvar_* cases (160 scenes) take 0.32 s; the slowest single case 0.15 s.
RUNTIME = {"test_gpu_fuzz.py + test_gpu_bvh.py fuzz, s": 1.11, "this module, s": 1.96, "its texvar_* cases, s": 0.32}


@pytest.mark.parametrize("hostile", [False, True], ids=["benign", "hostile"])
@pytest.mark.parametrize("name", list(FS.LANES))
def test_lane_matches_oracle(name, hostile, sky, oracle):
    from simple_raytracer_amd import build, tracer as T
    build.build_hip()
    iterations = FS.lane_iterations(name, int(os.environ.get("SRT_FUZZ_ITERS", "300")))  # soak runs: tests/fuzz_soak.py with SRT_FUZZ_LANE
    failures, classes, edits = FS.run_lane(T, oracle, sky, name, hostile, iterations)
    assert not failures, failures  # (lane, iteration, what, differing pixels, differing counters)
    # coverage: a class lane ran its class's kernel on EVERY iteration; the near misses had every edit
    assert len(classes) == iterations
    if name in FS.CLASS_LANES:
        assert classes == [FS.CLASS_LANES[name]] * iterations
    elif name == "near_miss":
        assert iterations < len(FS.NEAR_MISS_KINDS) or sorted(edits) == sorted(FS.NEAR_MISS_KINDS)  # (a shortened run: SRT_FUZZ_ITERS < 50)
        assert min(edits.values()) >= min(5, iterations // len(FS.NEAR_MISS_KINDS)), edits
        assert set(classes) <= {FS.GENERAL, FS.PPS_SPECULAR}
    else:
        assert set(classes) == {FS.GENERAL}
