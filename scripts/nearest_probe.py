"""What a nearest-surface query costs (include/srt_abi.h "nearest-surface queries"), next to the cast of as many rays. One JSON
document:

  rows      per scene -- the bench sphere scene, the two 968-triangle meshes, the 99,904-triangle mesh -- per acceleration mode
            (array scan, host SAH tree, device median tree; the sphere scene has no model, so one mode), per count (518,400 and
            2,073,600: the pixels of a 960x540 and a 1920x1080 frame) and per query set:
              surface   the hit points of the frame's pixel-centre rays (srt_pick over the frame), moved 0.05 along the normal;
                        a pixel that sees the sky gives the point 8 along its ray. Coherent and near the surface: snapping.
              random    uniform in the scene's box (spheres and model boxes), grown by a quarter each way.
            srt_nearest_points_device under the kernel timers (srt_last_ray_query_ms), REPS launches after one that warms up:
            median, min and max. Beside it srt_cast_rays_device of the frame's pixel-centre rays -- the same count -- in the same
            mode, measured the same way in a process of its own on the library --parent-lib names (a build of the parent commit;
            default: this one, whose cast kernels are the parent's instruction for instruction). nearest / cast per row, with
            the range the two spreads allow; "no claim" where that range holds 1.0. `same_as_scan`: the row's records equal the scan's of the
            same queries byte for byte (the contract, here at a scale no test runs).
  tree_over_scan   per scene with models, count and set: tree median / scan median, with the same range and "no claim" rule.
  one_point        the blocking time of a one-point srt_nearest_points (upload, launch, read-back), median of 50.

    python scripts/nearest_probe.py [--parent-lib PATH] [--out FILE] [--quick]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

REPS = 5
SIZES = [(960, 540), (1920, 1080)]
MODES = ("scan", "sah", "median")
F = np.float32


def med(xs):
    return float(statistics.median(xs))


def scenes():
    from simple_raytracer_amd import scenes as S
    return [("spheres", S.sphere_scene(), ("scan",)), ("mesh2", S.mesh_scene(), MODES), ("mesh100k", S.mesh_scene(1, 224, 224), MODES)]


def handle(scn, mode, w=960, h=540):
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    shapes, tris, mats = scn
    t = Tracer(w, h)
    t.set_acceleration(0 if mode == "scan" else 1)
    if mode == "median":
        t.set_acceleration_build(1, 0)
        t.set_acceleration_build_order(1)
    t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.set_kernel_timers(True)
    return t


def centre_rays(R, cam, w, h):
    """RAY records of the pixel centres of a w x h frame (scripts/ray_query_probe.py)"""
    px, py = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    ndc_x, ndc_y = (px.ravel() + F(0.5)) / F(w), (py.ravel() + F(0.5)) / F(h)
    sx = ((F(2) * ndc_x - F(1)) * (F(w) / F(h))).astype(F)
    sy = (F(1) - F(2) * ndc_y).astype(F)
    v = (cam[0, :3][None] * sx[:, None] + cam[1, :3][None] * sy[:, None]) - cam[2, :3][None]
    v = (v / np.sqrt((v * v).sum(axis=1, dtype=F))[:, None]).astype(F)
    return R.rays(cam[3, :3], v)


def query_sets(t, scn, w, h):
    from simple_raytracer_amd import records as R, scenes as S
    shapes = scn[0]
    cam = S.default_camera()
    rays = centre_rays(R, cam, w, h)
    xy = np.stack(np.meshgrid(np.arange(w, dtype=F) + F(0.5), np.arange(h, dtype=F) + F(0.5)), -1).reshape(-1, 2)
    hits = t.pick(xy, options=R.render_data(w, h, 2, 10, camera_to_world=cam))
    hit = (hits["flags"] & R.HIT_HIT) != 0
    tt = np.where(hit, hits["t"], F(8)).astype(F)
    surface = (rays["origin"] + rays["direction"] * tt[:, None] + hits["normal"] * F(0.05)).astype(F)
    lo, hi = [], []
    for s in shapes:
        if s["type"] == R.SHAPE_SPHERE:
            lo.append(s["sphere_position"] - abs(float(s["sphere_radius"]))), hi.append(s["sphere_position"] + abs(float(s["sphere_radius"])))
        elif s["type"] == R.SHAPE_MODEL and s["num_triangles"]:
            lo.append(s["bounding_min"]), hi.append(s["bounding_max"])
    lo, hi = np.min(lo, axis=0).astype(np.float64), np.max(hi, axis=0).astype(np.float64)
    grow = 0.25 * (hi - lo)
    random = np.random.default_rng(w * 31 + h).uniform(lo - grow, hi + grow, (w * h, 3)).astype(F)
    return {"surface": surface, "random": random}, int(hit.sum())


def timed(call, ms_of):
    ms = []
    for rep in range(REPS + 1):  # the first warms up
        call()
        ms.append(ms_of())
    ms = ms[1:]
    return {"median_ms": round(med(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def cast_child(quick):
    """the casts, on whatever library SRT_LIB names: one JSON line per (scene, mode, size)"""
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    dev = torch.device("cuda", 0)
    for name, scn, modes in scenes():
        for mode in modes:
            t = handle(scn, mode)
            for w, h in SIZES[:1] if quick else SIZES:
                rays = centre_rays(R, S.default_camera(), w, h)
                n = len(rays)
                rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
                hits_dev = torch.zeros((n, 8), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                r = timed(lambda: t.cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True), t.last_ray_query_ms)
                print(json.dumps({"scene": name, "mode": mode, "n": n, **r}), flush=True)
            t.close()


def ratio(a, b):
    """a / b of two timed() results: the medians' ratio, the range the spreads allow, and whether that range leaves 1.0 out"""
    lo, hi = a["min_ms"] / b["max_ms"], a["max_ms"] / b["min_ms"]
    return {"ratio": round(a["median_ms"] / b["median_ms"], 3), "range": [round(lo, 3), round(hi, 3)], "claim": not (lo <= 1.0 <= hi)}


def nearest_rows(quick, casts):
    import torch
    import srt_pkg
    srt_pkg.load()
    dev = torch.device("cuda", 0)
    rows, scan_digest, one_point = [], {}, {}
    for name, scn, modes in scenes():
        for mode in modes:
            t0 = time.perf_counter()
            t = handle(scn, mode)
            t.synchronize()
            setup_s = time.perf_counter() - t0
            for w, h in SIZES[:1] if quick else SIZES:
                sets, pixels_hit = query_sets(t, scn, w, h)
                for set_name, pts in sets.items():
                    n = len(pts)
                    q = np.zeros((n, 4), F)
                    q[:, :3], q[:, 3] = pts, np.inf
                    q_dev = torch.from_numpy(q.view(np.int32)).to(dev)
                    out_dev = torch.zeros((n, 8), dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    r = timed(lambda: t.nearest_points_device(q_dev.data_ptr(), n, out_dev.data_ptr()), t.last_ray_query_ms)
                    out = out_dev.cpu().numpy()
                    digest = hashlib.sha256(out.tobytes()).hexdigest()
                    if mode == "scan":
                        scan_digest[(name, n, set_name)] = digest
                    dist = out[:, 0].copy().view(F)
                    row = {"scene": name, "mode": mode, "n": n, "set": set_name, **r, "ns_per_query": round(r["median_ms"] * 1e6 / n, 3),
                           "found": int((out.view(np.uint32)[:, 7] & 1).sum()), "median_distance": round(float(np.median(dist)), 4),
                           "same_as_scan": digest == scan_digest[(name, n, set_name)], "setup_s": round(setup_s, 2), "pixels_hit": pixels_hit}
                    cast = casts.get((name, mode, n))
                    if cast:
                        row["cast"] = cast
                        row["nearest_over_cast"] = ratio(r, cast)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            blocking = []
            p = np.asarray(sets["surface"][len(sets["surface"]) // 2], F)
            for k in range(60):
                t1 = time.perf_counter()
                t.nearest_points(p + F(1e-3 * k))
                blocking.append(time.perf_counter() - t1)
            one_point[f"{name}/{mode}"] = round(med(blocking[10:]) * 1e3, 4)
            assert t.counters()["watchdog"] == 0
            t.close()
    return rows, one_point


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit, for the casts")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="518,400 queries only")
    ap.add_argument("--cast-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.cast_child:
        cast_child(a.quick)
        return
    env = dict(os.environ)
    env.pop("SRT_LIB", None)
    if a.parent_lib:
        env["SRT_LIB"] = str(Path(a.parent_lib).resolve())
    r = subprocess.run([sys.executable, __file__, "--cast-child"] + (["--quick"] if a.quick else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"the casts failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    casts = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            c = json.loads(line)
            casts[(c["scene"], c["mode"], c["n"])] = {k: c[k] for k in ("median_ms", "min_ms", "max_ms")}
            print("cast " + line, flush=True)
    rows, one_point = nearest_rows(a.quick, casts)
    by = {(x["scene"], x["mode"], x["n"], x["set"]): x for x in rows}
    tree_over_scan = []
    for (scene, mode, n, s), x in by.items():
        if mode != "scan":
            tree_over_scan.append({"scene": scene, "mode": mode, "n": n, "set": s, **ratio(x, by[(scene, "scan", n, s)])})
    doc = {"reps": REPS, "cast_library": "parent" if a.parent_lib else "this", "rows": rows, "tree_over_scan": tree_over_scan, "one_point_blocking_ms": one_point}
    print(json.dumps({"tree_over_scan": tree_over_scan, "one_point_blocking_ms": one_point}), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
