#!/usr/bin/env python3
"""What X-ray area selection costs (csrc/area_through.hip), on the device. The handle is bound to a stream of
the caller's (srt_bind_stream), so every time below but the host column is a DEVICE time: a timed span of the library's or two
events recorded on that stream around the launches, with no host wait between them. Per row -- frame, area, scene, acceleration
mode -- the median of REPS runs behind a warm-up run, the runs' minimum and maximum beside it:

  through    srt_area_coverage_through_device: the clear, the counting kernel and the finish kernel (srt_last_area_ms)
  visible    srt_area_coverage_device with a FRESH ID pass: the ID pass (events on the handle's stream around render_ids) plus
             the visible call's srt_last_area_ms -- what seeing through costs over seeing
  multi_k8   the only way the parent library has to approximate the through counts: srt_cast_rays_multi_device at k = 8 with
             SRT_RAYS_COUNT_ALL over the area's pixel rays (srt_last_ray_query_ms). THIS PATH IS INCOMPLETE beyond 8 candidates
             per ray: a dense mesh fills all eight slots with its own triangles; `truncated_rays` counts such rays
  host       that path's host part, wall clock, three runs: the read-back of ALL records (256 B per pixel) and counts, and a
             vectorised numpy de-duplication of ALL rays into per-shape counts (sort the eight shape words of a ray, count the
             first of each run)
  triangles  srt_area_triangle_coverage_through of the row's first model (rows with a model)

A ratio is given only where the two medians differ by more than the larger of the two spreads (max - min), else "no claim".
Rows: 960x540 and 1920x1080; the full frame and a 200x150 marquee; the bench sphere scene, the two 968-triangle meshes and the
99,904-triangle mesh, the meshes under the array scan and the SAH tree. --quick: 960x540 without the large mesh, REPS 3. One JSON
document on stdout (or --out)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402


def stats(xs):
    return {"median_ms": round(float(statistics.median(xs)), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def verdict(a, b):
    """a against b: the ratio of the medians, or "no claim" inside the run-to-run spread"""
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    if abs(a["median_ms"] - b["median_ms"]) <= spread or b["median_ms"] == 0:
        return "no claim"
    return round(a["median_ms"] / b["median_ms"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import srt_pkg
    srt_pkg.load()
    import torch
    from simple_raytracer_amd import records as R, scenes as S, tracer as T
    reps = 3 if args.quick else 5
    frames = [(960, 540)] if args.quick else [(960, 540), (1920, 1080)]
    scenes = {"spheres": S.sphere_scene(), "meshes_968": S.mesh_scene()}
    if not args.quick:
        scenes["mesh_99904"] = S.mesh_scene(1, 224, 224, smooth=False)
    stream = torch.cuda.Stream()
    rows = []
    for (w, h) in frames:
        for name, (sh, tr, ma) in scenes.items():
            for accel in ((0,) if name == "spheres" else (0, 1)):
                t = T.Tracer(w, h)
                t.bind_stream(stream.cuda_stream)
                t.set_acceleration(accel)
                t.set_kernel_timers(True)
                t.options = R.render_data(w, h, 1, 2, camera_to_world=S.default_camera(), time=777)
                t.scene_data = R.scene_data(len(sh))
                t.update_scene(sh, tr, ma)
                n = len(sh)
                dev = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
                models = np.flatnonzero(sh["type"] == R.SHAPE_MODEL)
                for label, rect in (("full", (0, 0, w, h)), ("marquee_200x150", (w // 2 - 100, h // 2 - 75, w // 2 + 100, h // 2 + 75))):
                    row = {"frame": [w, h], "area": label, "scene": name, "accel": "sah" if accel else "scan", "triangles": int(sh["num_triangles"][models].sum()) if len(models) else 0}
                    thr, vis, mk8, host, tri = [], [], [], [], []
                    ys, xs = np.mgrid[rect[1]:rect[3], rect[0]:rect[2]]
                    xy = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
                    rays_dev = torch.from_numpy(t.pick_rays(xy).view(np.int32).reshape(len(xy), 8).copy()).cuda()
                    hits_dev = torch.zeros((len(xy) * 8, 8), dtype=torch.int32, device="cuda")
                    cnt_dev = torch.zeros(len(xy), dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    for r in range(reps + 1):  # the first run warms up and is dropped
                        t.area_coverage_device(dev.data_ptr() + 32, n, dev.data_ptr(), rect, through=True)
                        thr.append(t.last_area_ms())
                        through_counts = dev.cpu().numpy()[8:8 + n].astype(np.int64)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)  # on the handle's stream, nothing waited for in between: a device span
                        t.render_ids()
                        e1.record(stream)
                        t.area_coverage_device(dev.data_ptr() + 32, n, dev.data_ptr(), rect, options=False)
                        area_ms = t.last_area_ms()  # (waits for the stream)
                        vis.append(e0.elapsed_time(e1) + area_ms)
                        t.cast_rays_multi_device(rays_dev.data_ptr(), len(xy), 8, hits_dev.data_ptr(), cnt_dev.data_ptr(), unit=True, count_all=True)
                        mk8.append(t.last_ray_query_ms())
                        if r <= 3:
                            c0 = time.perf_counter()
                            shapes = hits_dev.cpu().numpy().view(np.uint32).reshape(len(xy), 8, 8)[:, :, 1]  # srt_ray_hit's shape word; SRT_HIT_NONE in the slots past the last hit
                            cc = cnt_dev.cpu().numpy()
                            srt = np.sort(shapes, axis=1)
                            first = np.ones(srt.shape, bool)
                            first[:, 1:] = srt[:, 1:] != srt[:, :-1]
                            keys = srt[first & (srt < n)]
                            approx = np.bincount(keys, minlength=n)
                            host.append((time.perf_counter() - c0) * 1e3)
                            row["truncated_rays"] = int((cc > 8).sum())
                            row["k8_counts_equal_through"] = bool(np.array_equal(approx, through_counts))
                        if len(models):
                            s0 = int(models[0])
                            t.area_triangle_coverage(s0, int(sh["num_triangles"][s0]), rect, through=True)
                            tri.append(t.last_area_ms())
                    row["through"], row["visible_fresh_ids"], row["multi_k8_device"] = stats(thr[1:]), stats(vis[1:]), stats(mk8[1:])
                    row["multi_k8_readback_and_dedup_host"] = stats(host[1:])
                    row["through_vs_visible"] = verdict(row["through"], row["visible_fresh_ids"])
                    row["through_vs_multi_k8_device_only"] = verdict(row["through"], row["multi_k8_device"])
                    if tri:
                        row["triangles_through"] = stats(tri[1:])
                    rows.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    if args.out:  # (kept as the rows come: a run that is cut short leaves what it had)
                        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                        Path(args.out).write_text(json.dumps({"partial": True, "rows": rows}, indent=1))
                    del rays_dev, hits_dev, cnt_dev
                t.close()
    doc = {"what": "X-ray area selection against the visible form and against the k = 8 multi-hit approximation (incomplete beyond 8 candidates)",
           "reps": reps, "triangle_atomics": "per lane, one atomic per accepted triangle; the wave-aggregated form was not tried", "rows": rows}
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
