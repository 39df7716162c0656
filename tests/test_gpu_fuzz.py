"""GPU: differential fuzzing of the HIP path against the CPU oracle on random — including
hostile — scenes: degenerate shapes (zero / negative radius, zero or huge normals, flat and
sliver triangles, empty models, unknown shape types, negative material indices), extreme
materials (ior 0, NaN / inf / negative parameters), rays starting inside everything,
cameras with odd matrices. Canvas must stay bit-identical (NaN == NaN), counters equal."""
import os

import numpy as np
import pytest

from conftest import bits_equal
from fuzz_scenes import random_scene  # noqa: F401 (the generator lives in tests/fuzz_scenes.py; test_gpu_bvh.py and the soak scripts import it from here)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hostile", [False, True])
def test_random_scenes_match_oracle(hostile, sky, oracle):
    from simple_raytracer_amd import build, tracer as T
    build.build_hip()
    rng = np.random.RandomState(20240 + int(hostile))
    w, h = 24, 16
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.count_triangles(True)
    failures = []
    for it in range(int(os.environ.get("SRT_FUZZ_ITERS", "300"))):  # soak runs: SRT_FUZZ_ITERS=3000
        shapes, tris, mats, cam = random_scene(rng, hostile)
        rd = R.render_data(w, h, int(rng.randint(1, 5)), int(rng.choice([1, 2, 5, 10])), fov_scale=float(rng.uniform(0.3, 2.0)),
                           camera_to_world=cam, time=int(rng.randint(1, 2**31)), show_normals=bool(rng.rand() < 0.1))
        sd = R.scene_data(len(shapes), sun_focus=float(rng.choice([25.0, 1.0, 32.0, 7.5, 0.0, 100.0])), sun_intensity=float(rng.uniform(0, 3)))
        t.options, t.scene_data = rd, sd
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        t.reset_counters()
        t.trace()
        got = t.read_canvas()
        c = t.counters()
        with np.errstate(all="ignore"):
            want, oc = oracle.render(rd, sd, shapes, tris, mats, sky, counters=True, nthreads=4)
        ok = bits_equal(got, want) and all(c[k] == oc[k] for k in ("paths", "rays", "sky", "tri_tests", "tri_pass_u", "nan_pixels")) and c["watchdog"] == 0
        if not ok:
            bad = int((~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).any(axis=-1).sum())
            failures.append((it, bad, {k: (c[k], oc[k]) for k in ("rays", "sky", "tri_tests", "tri_pass_u", "nan_pixels") if c[k] != oc[k]}))
    t.close()
    assert not failures, failures
