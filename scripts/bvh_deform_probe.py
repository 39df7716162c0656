"""Cost of srt_update_scene under SRT_ACCEL_BVH when a model's VERTICES change: rebuilt (SRT_DEFORM_REBUILD, the default) against
kept and refitted (SRT_DEFORM_REFIT), with the refit on the host and on the device, for the 10^5-triangle mesh and the two
1k-triangle meshes. Every model is displaced by a smooth wave of a few percent of its size per step, --steps steps (32). Wall
time from the call to the end of srt_synchronize; the cost ratio after every step; the device time of the refit launches
with the cost launch behind them from the library's event pair (bvh_device_refit_probe.py has the refit launches alone);
the trace time of one 960x540x2-spp frame at the last step on the refitted tree and, in the rebuild run, on a tree built
from the last step's mesh. A library without
srt_set_acceleration_deform (an earlier build, run from its own tree) reports the rebuild figures only. One JSON line.
usage: bvh_deform_probe.py [--steps N]"""
import json, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import srt_pkg
srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S
from simple_raytracer_amd.tracer import Tracer

STEPS = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 32
HAS_DEFORM = hasattr(Tracer, "set_acceleration_deform")
SKY = S.synthetic_sky()


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def waved(tris, k, amplitude=0.03):
    """every vertex + a * sin(k . p + phase), a = 3 % of the array's diagonal, phase moving with the step; normals stay"""
    out = tris.copy()
    p = np.asarray(tris["v"]["pos"], np.float64)[..., :3]
    flat = p.reshape(-1, 3)
    diag = float(np.sqrt(((flat.max(axis=0) - flat.min(axis=0)) ** 2).sum()))
    kvec = np.array([[2.1, 0.7, -1.3], [-0.9, 1.9, 0.8], [1.1, -1.4, 2.3]]) * (2.0 * np.pi / diag)
    out["v"]["pos"][..., :3] = (p + amplitude * diag * np.sin(p @ kvec.T + np.array([0.3, 1.1, 2.0]) + 0.2 * k)).astype(np.float32)
    return out


def timed_update(t, shapes, tris, mats):
    t0 = time.perf_counter()
    t.update_scene(shapes, tris, mats)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def trace_ms(t, reps=5):
    out = []
    for _ in range(reps):
        t.clear_canvas()
        t.trace()
        out.append(t.last_kernel_ms()[0])
    return stats(out)


def probe(scene):
    shapes, tris, mats = scene
    tris = R.as_records(tris, R.TRIANGLE)
    meshes = [waved(tris, k) for k in range(1, STEPS + 1)]
    res = {"triangles": int(sum(int(s["num_triangles"]) for s in shapes if s["type"] == 2))}
    modes = [("rebuild", 0, 0)] + ([("refit_host", 1, 0), ("refit_device", 1, 1)] if HAS_DEFORM else [])
    for name, deform, refit in modes:
        t = Tracer(960, 540)
        t.set_skybox(SKY)
        t.set_acceleration(1)
        if HAS_DEFORM:
            t.set_acceleration_refit(refit)
            t.set_acceleration_deform(deform)
        t.set_kernel_timers(True)
        t.scene_data = R.scene_data(len(shapes))
        t.options = R.render_data(960, 540, 2, 10, camera_to_world=S.default_camera(), time=31337)
        build = timed_update(t, shapes, tris, mats)
        ms, kern, ratio = [], [], []
        for m in meshes:
            ms.append(timed_update(t, shapes, m, mats))
            if refit:
                kern.append(t.last_refit_kernel_ms())
            if deform:
                ratio.append(round(t.acceleration_deform_info()["worst_ratio"], 6))
        r = {"build_ms": round(build, 3), "deformed_ms": stats(ms), "trace_ms_last_step": trace_ms(t), "acceleration_info": t.acceleration_info()}
        if deform:
            r["ratio_per_step"] = ratio
            r["deform_info"] = t.acceleration_deform_info()
        if refit:
            r["refit_and_cost_kernels_ms"] = stats(kern)
        res[name] = r
        t.close()
    return res


print(json.dumps({"deform_refit_available": HAS_DEFORM, "steps": STEPS, "mesh100k": probe(S.mesh_scene(1, 224, 224, smooth=False)), "mesh2x1k": probe(S.mesh_scene(2))}))
