"""Device time of the denoiser's temporal stage (srt_set_denoise_temporal) at 960x540 and 1920x1080, and the quality of a
moving camera against history_limit.

  setup_spatial_ms     srt_resolve_denoised with K = 0, temporal off: the spatial set-up and the tonemap (library HIP events)
  setup_identity_ms    the same with temporal on and the history taken by the same camera (one tap per pixel)
  setup_moved_ms       temporal on, the camera moved since the history (the bilinear 2x2 reprojection)
  clear_wall_ms        host clock around srt_clear_canvas + synchronise, temporal off (the canvas and sums zeroed)
  commit_wall_ms       the same with temporal on after a trace and no filter: the clear also integrates the frame (one launch
                       of the set-up kernel without its outputs for the filter) and swaps the history sets
  commit_fresh_wall_ms the same after a filter: the clear only swaps the sets

Medians over --reps. Scene: the sphere scene, 2 spp. --quality adds, for history_limit 8, 16, 32 and 64, the tonemapped MSE of
the last of 8 moving frames at 2 spp (160x90, spheres and meshes) against a 4096-spp image at its camera, temporal over
spatial, and the same over the pixels with a first hit and without history (disoccluded). Writes one JSON per size (profiles/r06_temporal_<w>x<h>.json)
and profiles/r06_temporal_quality.json to --out-dir.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import build as B, records as R, scenes as S, tracer as TR  # noqa: E402


def handle(w, h, spp, name, accel=0):
    shapes, tris, mats = S.sphere_scene() if name == "spheres" else S.mesh_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t


def cam_at(k):
    return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)


def resolve_ms(t, reps):
    out = []
    for _ in range(reps):
        t.resolve_denoised(1)
        out.append(t.last_kernel_ms()[1])
    return statistics.median(out[1:])


def clear_ms(t, reps, filtered):
    out = []
    for i in range(reps):
        t.options["time"] = 500 + i
        t.trace()
        if filtered:
            t.resolve_denoised(1)
        t.synchronize()
        t0 = time.perf_counter()
        t.clear_canvas()
        t.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out[1:])


def probe(w, h, spp, reps):
    t = handle(w, h, spp, "spheres")
    t.set_denoise(iterations=0)
    t.trace()
    r = {"width": w, "height": h, "spp": spp, "reps": reps, "setup_spatial_ms": resolve_ms(t, reps)}
    r["clear_wall_ms"] = clear_ms(t, reps, False)
    t.set_denoise_temporal()
    t.trace()
    t.clear_canvas()  # the history: the same camera
    t.trace()
    r["setup_identity_ms"] = resolve_ms(t, reps)
    t.clear_canvas()
    t.options["camera_to_world"] = cam_at(1)
    t.trace()
    r["setup_moved_ms"] = resolve_ms(t, reps)
    r["commit_wall_ms"] = clear_ms(t, reps, False)
    r["commit_fresh_wall_ms"] = clear_ms(t, reps, True)
    px = w * h
    # traffic of the moved set-up per pixel: canvas, sums, moments in (52 B); history taps (up to 4 x 56 B, mostly cache hits
    # between neighbours: 56 B from DRAM); out {c, V}, staging set (16 + 8 + 32 B) and argb out (4 B)
    r["bytes_per_pixel_min"] = 52 + 56 + 16 + 56 + 4
    r["effective_GBps_moved"] = r["bytes_per_pixel_min"] * px / (r["setup_moved_ms"] * 1e-3) / 1e9
    t.close()
    return r


def tone(x):
    a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    x = np.asarray(x, np.float64)
    return np.sqrt(np.clip((x * (x * a + b)) / (x * (x * c + d) + e), 0, 1))


def quality(limits, frames=8):
    w, h = 160, 90
    res = {}
    for name, accel in (("spheres", 0), ("meshes", 1)):
        g = handle(w, h, 4096, name, accel)
        g.options["camera_to_world"] = cam_at(frames - 1)
        g.options["time"] = 4242
        g.render(1)
        ref = tone(g.read_canvas()[..., :3])
        g.close()
        shapes, tris, mats = S.sphere_scene() if name == "spheres" else S.mesh_scene()
        runs = {}
        for limit in [None] + list(limits):
            t = handle(w, h, 2, name, accel)
            t.set_denoise()
            if limit:
                t.set_denoise_temporal(history_limit=limit)
            for k in range(frames):
                t.clear_canvas()
                t.update_scene(shapes, tris, mats)
                t.options["camera_to_world"] = cam_at(k)
                t.options["time"] = 900 + k
                t.render(1)
            out = tone(t.read_denoised()[..., :3])
            dis = None
            if limit:
                t.clear_canvas()
                hist = t.read_denoise_history()
                dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)  # a first hit, and no history reached it
            runs[limit] = (out, dis)
            t.close()
        sp = runs[None][0]
        mse_s = float(np.mean((sp - ref) ** 2))
        r = {"spatial_mse": mse_s}
        for limit in limits:
            out, dis = runs[limit]
            r[str(limit)] = {"mse_ratio": float(np.mean((out - ref) ** 2)) / mse_s,
                             "disoccluded_fraction": float(dis.mean()),
                             "disoccluded_mse_ratio": float(np.mean((out[dis] - ref[dis]) ** 2)) / float(np.mean((sp[dis] - ref[dis]) ** 2))}
        res[name] = r
        print(name, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    B.build_hip()
    for s in a.sizes.split(","):
        if not s:
            continue
        w, h = (int(v) for v in s.split("x"))
        res = probe(w, h, a.spp, a.reps)
        print(json.dumps(res), flush=True)
        if a.out_dir:
            p = Path(a.out_dir) / f"r06_temporal_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))
    if a.quality:
        q = quality((8, 16, 32, 64))
        if a.out_dir:
            (Path(a.out_dir) / "r06_temporal_quality.json").write_text(json.dumps(q, indent=1))


if __name__ == "__main__":
    main()
