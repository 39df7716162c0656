"""Cost of srt_update_scene under SRT_ACCEL_BVH when a model only moves, with the refit on the host (SRT_REFIT_HOST, the default)
and on the device (SRT_REFIT_DEVICE), for the 10^5-triangle mesh and the two 1k-triangle meshes. Wall time from the call to
the end of srt_synchronize (the device mode moves work onto the stream, so the sync belongs inside the span); the refit
launches' own time from the library's event pair; the trace time of one 960x540x2-spp frame on the host-refitted and on the
device-refitted hierarchy after the same rotation. A library without srt_set_acceleration_refit (an earlier build, run
from its own tree) reports the host figures only. One JSON line: medians and (min, max) over --reps moves.
usage: bvh_device_refit_probe.py [--reps N]"""
import json, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import srt_pkg
srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S
from simple_raytracer_amd.tracer import Tracer

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
HAS_DEVICE = hasattr(Tracer, "set_acceleration_refit")
SKY = S.synthetic_sky()


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def moved(shapes, k):
    """every model rotated and shifted a little further: same triangles, another transform"""
    out = shapes.copy()
    for i in range(len(out)):
        if out[i]["type"] == 2:
            out[i]["transform"] = R.mat_mul(R.translate((0.01 * k, 0.0, 0.0)), R.mat_mul(np.asarray(shapes[i]["transform"], np.float32), R.euler_yxz(0.05 * k, 0.02 * k, 0.0)))
    return out


def timed_update(t, shapes, tris, mats):
    t0 = time.perf_counter()
    t.update_scene(shapes, tris, mats)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def probe(scene):
    shapes, tris, mats = scene
    res = {"triangles": int(sum(int(s["num_triangles"]) for s in shapes if s["type"] == 2))}
    for mode in (("host", "device") if HAS_DEVICE else ("host",)):
        t = Tracer(960, 540)
        t.set_skybox(SKY)
        t.set_acceleration(1)
        if HAS_DEVICE:
            t.set_acceleration_refit(1 if mode == "device" else 0)
        t.set_kernel_timers(True)
        t.scene_data = R.scene_data(len(shapes))
        t.options = R.render_data(960, 540, 2, 10, camera_to_world=S.default_camera(), time=31337)
        build = timed_update(t, shapes, tris, mats)
        unchanged = [timed_update(t, shapes, tris, mats) for _ in range(REPS)]
        mv, kern, trace = [], [], []
        for k in range(1, REPS + 1):
            mv.append(timed_update(t, moved(shapes, k), tris, mats))
            if mode == "device":
                kern.append(t.last_refit_kernel_ms())
            t.clear_canvas()
            t.trace()
            trace.append(t.last_kernel_ms()[0])
        r = {"build_ms": round(build, 3), "unchanged_ms": stats(unchanged), "moved_ms": stats(mv), "trace_ms_after_move": stats(trace)}
        if mode == "device":
            r["refit_kernels_ms"] = stats(kern)
            r["refit_info"] = t.acceleration_refit_info()
        res[mode] = r
        t.close()
    return res


print(json.dumps({"device_refit_available": HAS_DEVICE, "reps": REPS, "mesh100k": probe(S.mesh_scene(1, 224, 224, smooth=False)), "mesh2x1k": probe(S.mesh_scene(2))}))
