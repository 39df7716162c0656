"""Cost of srt_update_scene under SRT_ACCEL_BVH for a NEW mesh -- other triangle bytes every time, so nothing is kept -- with the
build on the host (SRT_BUILD_HOST, the default: binned SAH) and on the device (SRT_BUILD_DEVICE: Morton sort under the balanced
topology), for bench.py's 99,904-triangle mesh scene, and for an unchanged scene as the floor. Wall time from the call to the
end of srt_synchronize (the device build moves work onto the stream, so the sync belongs inside the span); the build launches'
own time from the library's event pair (srt_last_build_kernel_ms: first build launch to the end of the refit behind it); the
trace kernel time of BASELINE configs[4] (the 99,904-triangle mesh) and configs[2] (two 968-triangle meshes) on the SAH tree
and on the Morton tree; and the two trees' surface-area cost on the host. A library without srt_set_acceleration_build (an
earlier build, run from its own tree) reports the host figures only. One JSON line: medians and (min, max) over --reps.
usage: bvh_build_probe.py [--reps N] [--spp-scale F]   (--spp-scale 0.25: a quarter of the configs' samples, for a short run)"""
import json, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import srt_pkg
srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S, tracer as T
from simple_raytracer_amd.tracer import Tracer

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
SPP_SCALE = float(sys.argv[sys.argv.index("--spp-scale") + 1]) if "--spp-scale" in sys.argv else 1.0
HAS_DEVICE = hasattr(Tracer, "set_acceleration_build")
SKY = S.synthetic_sky()
CONFIGS = {"configs4_mesh100k_1080p_256spp": (lambda: S.mesh_scene(1, 224, 224, smooth=False), 256),
           "configs2_meshes_1080p_512spp": (lambda: S.mesh_scene(2), 512)}


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def nudged(tris, k):
    """the same mesh with every vertex a hair elsewhere: other bytes, so no hierarchy of the previous call matches"""
    out = R.as_records(tris, R.TRIANGLE).copy()
    out["v"]["pos"][..., 0] += np.float32(1e-4 * k)
    return out


def timed_update(t, shapes, tris, mats):
    t0 = time.perf_counter()
    t.update_scene(shapes, tris, mats)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def handle(mode, w=960, h=540):
    t = Tracer(w, h)
    t.set_skybox(SKY)
    t.set_acceleration(1)
    if HAS_DEVICE:
        t.set_acceleration_build(1 if mode == "device" else 0)
    t.set_kernel_timers(True)
    return t


def update_costs():
    shapes, tris, mats = S.mesh_scene(1, 224, 224, smooth=False)
    res = {"triangles": int(sum(int(s["num_triangles"]) for s in shapes if s["type"] == 2))}
    for mode in (("host", "device") if HAS_DEVICE else ("host",)):
        t = handle(mode)
        t.scene_data = R.scene_data(len(shapes))
        first = timed_update(t, shapes, tris, mats)
        unchanged = [timed_update(t, shapes, tris, mats) for _ in range(REPS)]
        new, kern = [], []
        for k in range(1, REPS + 1):
            new.append(timed_update(t, shapes, nudged(tris, k), mats))
            if mode == "device":
                kern.append(t.last_build_kernel_ms())
        r = {"first_ms": round(first, 3), "unchanged_ms": stats(unchanged), "new_mesh_ms": stats(new), "host_build_us": t.acceleration_info()["build_us"]}
        if mode == "device":
            r["build_kernels_ms"] = stats(kern)
            r["build_info"] = t.acceleration_build_info()
        res[mode] = r
        t.close()
    return res


def trace_times():
    out = {}
    for name, (make, spp) in CONFIGS.items():
        shapes, tris, mats = make()
        spp = max(1, int(spp * SPP_SCALE))
        r = {"spp": spp}
        for mode in (("host", "device") if HAS_DEVICE else ("host",)):
            t = handle(mode, 1920, 1080)
            t.scene_data = R.scene_data(len(shapes))
            t.options = R.render_data(1920, 1080, spp, 10, camera_to_world=S.default_camera(), time=31337)
            t.update_scene(shapes, tris, mats)
            ms = []
            for _ in range(3):
                t.clear_canvas()
                t.trace()
                ms.append(t.last_kernel_ms()[0])
            r[mode + "_tree_trace_ms"] = stats(ms[1:])
            t.close()
        if HAS_DEVICE:
            r["trace_ratio_morton_over_sah"] = round(r["device_tree_trace_ms"]["median"] / r["host_tree_trace_ms"]["median"], 4)
            sah = morton = 0.0
            for s in shapes:  # the costs of the scene's models, summed
                if s["type"] == 2:
                    sah += T.bvh_wide_cost_host(s, tris, s, tris)[0]
                    morton += T.bvh_morton_wide_host(s, tris)["cost"]
            r["wide_cost"] = {"sah": round(sah, 4), "morton": round(morton, 4), "ratio": round(morton / sah, 4)}
        out[name] = r
    return out


print(json.dumps({"device_build_available": HAS_DEVICE, "reps": REPS, "spp_scale": SPP_SCALE, "update_mesh100k": update_costs(), "trace": trace_times()}))
