"""What the ORDER of a device-built hierarchy costs and buys: srt_update_scene under SRT_ACCEL_BVH for a NEW mesh (other triangle
bytes every time, so nothing is kept) and the trace kernel on the tree it leaves, for three settings -- SRT_BUILD_HOST (binned
SAH), SRT_BUILD_DEVICE with SRT_BUILD_ORDER_MORTON, and SRT_BUILD_DEVICE with SRT_BUILD_ORDER_MEDIAN. One worker process with one
handle per setting; the parent alternates the settings within every repetition, so drift hits all three alike. Meshes: bench.py's
99,904-triangle mesh scene (BASELINE configs[4]) and the scene of two 968-triangle meshes (configs[2]).
Per setting and mesh: wall time from the call to the end of srt_synchronize for a new mesh, and the host pass's part of it
(srt_acceleration_info's build time); the build launches' count and their time from the library's event pair
(srt_last_build_kernel_ms: first build launch to the end of the refit behind it); the trace kernel time of the config on the
tree; and the tree's surface-area cost from the host statements. One JSON line: medians and (min, max) over --reps.
usage: bvh_build_order_probe.py [--reps N] [--spp-scale F]   (--spp-scale 0.25: a quarter of the configs' samples, for a short run)"""
import json, subprocess, sys, time
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
SETTINGS = {"host_sah": (T.BUILD_HOST, T.BUILD_ORDER_MORTON), "device_morton": (T.BUILD_DEVICE, T.BUILD_ORDER_MORTON), "device_median": (T.BUILD_DEVICE, T.BUILD_ORDER_MEDIAN)}
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


def worker(setting):
    """one handle; a command per line on stdin, a JSON line per command on stdout"""
    mode, order = SETTINGS[setting]
    t = Tracer(1920, 1080)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(1)
    t.set_acceleration_build(mode)
    t.set_acceleration_build_order(order)
    t.set_kernel_timers(True)
    scenes = {name: make() for name, (make, _) in CONFIGS.items()}
    for line in sys.stdin:
        cmd, name, k = line.split()
        shapes, tris, mats = scenes[name]
        t.scene_data = R.scene_data(len(shapes))
        if cmd == "update":  # a new mesh: nothing to keep
            new = nudged(tris, int(k))
            t0 = time.perf_counter()
            t.update_scene(shapes, new, mats)
            t.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            out = {"ms": ms, "host_ms": t.acceleration_info()["build_us"] / 1e3, "kernels_ms": t.last_build_kernel_ms(), "launches": t.acceleration_build_info()["launches"]}
        elif cmd == "load":  # the config's own scene, and a trace to warm up
            spp = max(1, int(CONFIGS[name][1] * SPP_SCALE))
            t.options = R.render_data(1920, 1080, spp, 10, camera_to_world=S.default_camera(), time=31337)
            t.update_scene(shapes, tris, mats)
            t.clear_canvas()
            t.trace()
            out = {"spp": spp, "ms": t.last_kernel_ms()[0]}
        elif cmd == "trace":
            t.clear_canvas()
            t.trace()
            out = {"ms": t.last_kernel_ms()[0]}
        else:
            break
        print(json.dumps(out), flush=True)
    t.close()


def costs(name):
    """the surface-area costs of the config's models, summed, per setting (host statements)"""
    shapes, tris, _ = CONFIGS[name][0]()
    c = {s: 0.0 for s in SETTINGS}
    balanced = 0.0
    for s in shapes:
        if s["type"] == 2:
            c["host_sah"] += T.bvh_wide_cost_host(s, tris, s, tris)[0]
            c["device_morton"] += T.bvh_morton_wide_host(s, tris)["cost"]
            c["device_median"] += T.bvh_median_wide_host(s, tris)["cost"]
            balanced += T.bvh_wide_cost_host(s, tris, s, tris, force_balanced=True)[0]
    out = {s: round(v, 4) for s, v in c.items()}
    out["host_balanced"] = round(balanced, 4)
    return out


def main():
    procs = {s: subprocess.Popen([sys.executable, __file__, "--worker", s], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for s in SETTINGS}

    def ask(s, *cmd):
        procs[s].stdin.write(" ".join(str(c) for c in cmd) + "\n")
        procs[s].stdin.flush()
        line = procs[s].stdout.readline()
        if not line:
            raise RuntimeError(f"worker {s} ended (exit status {procs[s].poll()})")
        return json.loads(line)

    res = {"reps": REPS, "spp_scale": SPP_SCALE, "settings": list(SETTINGS), "meshes": {}}
    try:
        for name in CONFIGS:
            for s in SETTINGS:
                ask(s, "update", name, 0)  # allocations, the topology of the count
            runs = {s: [] for s in SETTINGS}
            for k in range(1, REPS + 1):
                for s in SETTINGS:
                    runs[s].append(ask(s, "update", name, k))
            spp = {s: ask(s, "load", name, 0)["spp"] for s in SETTINGS}
            traces = {s: [] for s in SETTINGS}
            for k in range(REPS):
                for s in SETTINGS:
                    traces[s].append(ask(s, "trace", name, k)["ms"])
            r = {"spp": spp["host_sah"], "wide_cost": costs(name)}
            for s in SETTINGS:
                r[s] = {"update_new_mesh_ms": stats([x["ms"] for x in runs[s]]), "update_host_part_ms": stats([x["host_ms"] for x in runs[s]]),
                        "build_kernels_ms": stats([x["kernels_ms"] for x in runs[s]]), "build_launches": runs[s][-1]["launches"], "trace_kernel_ms": stats(traces[s])}
            for s in ("device_morton", "device_median"):
                r[s]["trace_over_sah"] = round(r[s]["trace_kernel_ms"]["median"] / r["host_sah"]["trace_kernel_ms"]["median"], 4)
                r[s]["cost_over_sah"] = round(r["wide_cost"][s] / r["wide_cost"]["host_sah"], 4)
            res["meshes"][name] = r
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit x 0\n")
                p.stdin.close()
            except OSError:
                pass
        for p in procs.values():
            p.wait(timeout=60)
    print(json.dumps(res))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()
