"""Host time per dispatch: the wall time of each blocking render() call (srt_render: trace + reduction that resolves + read-back)
of the interactive frame, 960x540 at 2 spp, 4000 calls after 500 of warm-up; prints one JSON line with the median, the 10th and
90th percentile and the mean in microseconds. scripts/interactive_probe.py times the same loop as a whole (a mean); this one
gives the median a comparison of two builds wants. SRT_LIB selects the library; usage: render_median_probe.py [label]"""
import json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import srt_pkg
srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S
from simple_raytracer_amd.tracer import Tracer

w, h, spp = 960, 540, 2
shapes, tris, mats = S.sphere_scene()
t = Tracer(w, h)
t.set_skybox(S.synthetic_sky())
t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera())
t.scene_data = R.scene_data(len(shapes))
t.update_scene(shapes, tris, mats)
out = np.zeros(w * h * 4, np.uint8)
t.clear_canvas()
for frame in range(500):
    t.render(frame + 1, out)
N = 4000
dts = np.zeros(N)
for frame in range(N):
    t.options["time"] = np.uint32(1000 + frame)
    t0 = time.perf_counter()
    t.render(frame + 1, out)
    dts[frame] = time.perf_counter() - t0
t.close()
res = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "lib": os.environ.get("SRT_LIB", "tree"), "frames": N,
       "median_us": round(float(np.median(dts)) * 1e6, 2), "p10_us": round(float(np.percentile(dts, 10)) * 1e6, 2),
       "p90_us": round(float(np.percentile(dts, 90)) * 1e6, 2), "mean_us": round(float(dts.mean()) * 1e6, 2),
       "checksum": int(out.astype(np.uint64).sum())}
print(json.dumps(res))
