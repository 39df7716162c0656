"""What a multi-hit query costs (include/srt_abi.h "multi-hit ray queries") beside the closest-hit cast. One JSON document:

  multi           the centre rays of a frame of the bench sphere scene, the two 968-triangle meshes and the 99,904-triangle mesh,
                  each under the array scan and under the SAH tree (the sphere scene has no models: one row; the 99,904-triangle
                  scan runs a 240x135 frame, the others 960x540), through srt_cast_rays_multi_device at k = 1, 2, 4, 8 and at
                  k = 8 with SRT_RAYS_COUNT_ALL, under the kernel timers (srt_last_ray_query_ms). With --parent-lib PATH, a build of
                  the parent commit: srt_cast_rays_device of that library on the same rays, once and k times in a row -- the
                  cheapest thing a front-end could attempt without this query, though it cannot give the answer -- measured in
                  a process of its own before and after this library's columns. Every column: median, min and max over REPS
                  runs. Every ratio: the medians' quotient and the interval [min / max, max / min]; where 1 lies inside the
                  interval the verdict is "no claim".
  pick_latency    the blocking time of a one-point srt_pick_through at k = 8 (upload, two launches, read-back) at 960x540,
                  beside a blocking one-point srt_pick on the same handle.

    python scripts/multi_hit_probe.py [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

from ray_query_probe import centre_rays  # noqa: E402

REPS = 5
KS = (1, 2, 4, 8)


def col(xs):
    return {"median": round(float(statistics.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def ratio(a, b):
    """a / b of two columns with the interval the runs' spread allows"""
    lo, hi = a["min"] / b["max"], a["max"] / b["min"]
    return {"ratio": round(a["median"] / b["median"], 3), "lo": round(lo, 3), "hi": round(hi, 3), "verdict": "no claim" if lo <= 1.0 <= hi else
            ("slower" if lo > 1.0 else "faster")}


def rows():
    from simple_raytracer_amd import scenes as S
    return [("spheres", S.sphere_scene(), 0, (960, 540)), ("mesh2_scan", S.mesh_scene(), 0, (960, 540)), ("mesh2_bvh", S.mesh_scene(), 1, (960, 540)),
            ("mesh100k_scan", S.mesh_scene(1, 224, 224), 0, (240, 135)), ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1, (960, 540))]


def handle(scn, accel, w, h):
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    shapes, tris, mats = scn
    t = Tracer(w, h)
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.set_kernel_timers(True)
    return t


def measure(cast_only):
    """this process's library (whatever SRT_LIB names) over the rows: the multi columns, or with cast_only the cast's"""
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    dev = torch.device("cuda", 0)
    out = {}
    for name, scn, accel, (w, h) in rows():
        t = handle(scn, accel, w, h)
        rays = centre_rays(R, S.default_camera(), w, h)
        n = len(rays)
        rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
        hits_dev = torch.zeros((n * 8, 8), dtype=torch.int32, device=dev)
        counts_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        row = {"rays": n}
        if cast_only:
            for k in KS:
                ms = []
                for rep in range(REPS + 1):  # the first warms up
                    total = 0.0
                    for _ in range(k):
                        t.cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True)
                        total += t.last_ray_query_ms()
                    ms.append(total)
                row[f"cast_x{k}_ms"] = col(ms[1:])
        else:
            for k, count_all in [(k, False) for k in KS] + [(8, True)]:
                ms = []
                for rep in range(REPS + 1):
                    t.cast_rays_multi_device(rays_dev.data_ptr(), n, k, hits_dev.data_ptr(), counts_dev.data_ptr(), unit=True, count_all=count_all)
                    ms.append(t.last_ray_query_ms())
                row["count_all_k8_ms" if count_all else f"k{k}_ms"] = col(ms[1:])
                if count_all:
                    c = counts_dev.cpu().numpy()
                    row["candidates_mean"], row["candidates_max"] = round(float(c.mean()), 3), int(c.max())
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        t.close()
    return out


def parent_columns(parent_lib):
    env = dict(os.environ)
    env["SRT_LIB"] = str(parent_lib)
    r = subprocess.run([sys.executable, __file__, "--cast-child"], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"the parent library's run failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def pick_latency():
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import scenes as S
    res = {}
    for name, scn, accel in (("spheres", S.sphere_scene(), 0), ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)):
        t = handle(scn, accel, 960, 540)
        picks, throughs = [], []
        for k in range(60):
            t0 = time.perf_counter()
            t.pick([[480.5 + k, 270.5]])
            picks.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            t.pick_through([[480.5 + k, 270.5]], 8)
            throughs.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"pick_ms": col(picks[10:]), "pick_through_k8_ms": col(throughs[10:])}
        res[name]["through_over_pick"] = ratio(res[name]["pick_through_k8_ms"], res[name]["pick_ms"])
        t.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit: the cast columns")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--cast-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.cast_child:
        print(json.dumps(measure(True)))
        return
    doc = {"reps": REPS}
    before = parent_columns(a.parent_lib) if a.parent_lib else None
    doc["multi"] = measure(False)
    if a.parent_lib:
        after = parent_columns(a.parent_lib)
        for name, row in doc["multi"].items():
            for k in KS:  # the parent's two runs, before and after, pooled: their drift is part of the spread
                b, c = before[name][f"cast_x{k}_ms"], after[name][f"cast_x{k}_ms"]
                row[f"parent_cast_x{k}_ms"] = {"median": round((b["median"] + c["median"]) / 2, 4), "min": min(b["min"], c["min"]), "max": max(b["max"], c["max"])}
            for k in KS:
                row[f"k{k}_over_parent_cast"] = ratio(row[f"k{k}_ms"], row["parent_cast_x1_ms"])
                row[f"k{k}_over_parent_cast_x{k}"] = ratio(row[f"k{k}_ms"], row[f"parent_cast_x{k}_ms"])
            row["count_all_over_k8"] = ratio(row["count_all_k8_ms"], row["k8_ms"])
    doc["pick_latency"] = pick_latency()
    print(json.dumps({"pick_latency": doc["pick_latency"]}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
