"""The denoiser's spatial variance estimate (srt_set_denoise_spatial_variance): device time and quality.

Time, from the library's own HIP events (srt_last_kernel_ms after srt_resolve_denoised), the filter with the switch off and
on (min_samples = 8) alternated in one process on one handle and one canvas, medians of --reps rounds after one that is
thrown away, in the library as built (the halo tile in LDS) and in the -DSRT_SV_GLOBAL variant (plain global loads):

  first frame   sphere scene, 2 spp, spatial set-up: every first hit qualifies
  eighth frame  the moving-camera sequence under temporal reprojection: only pixels with fewer than 8 samples qualify
  estimate_ms   filter(K = 5, on) - filter(K = 5, off): the new launch
  pass_ms       (filter(K = 5, off) - filter(K = 1, off)) / 4: one a-trous pass of the same run
  early_out     the share of 16x16 tiles none of whose pixels qualifies (from the read-backs, on the host)

Quality at 160x90 against 4096 spp, tonemapped MSE, switch on / switch off (tests/test_gpu_denoise_spatial_variance.py's
protocol): the first 2-spp frame after a clear, and the eighth frame of the moving-camera sequence over the whole frame and
over the pixels that had no history in that frame.

Writes profiles/r18_spatial_variance_<w>x<h>.json and profiles/r18_spatial_variance_quality.json to --out-dir.
"""
import argparse
import ctypes as C
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

MIN_SAMPLES = 8
GLOBAL_LIB = B.LIBDIR / "variants" / "sv_global" / "libsrt_hip.so"


def cam_at(k):
    return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)


def handle(w, h, spp, name, accel, lib=None, time_=1234):
    shapes, tris, mats = S.sphere_scene() if name == "spheres" else S.mesh_scene()
    t = TR.Tracer(w, h, lib=lib)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=time_)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.scene = (shapes, tris, mats)
    return t


def next_frame(t, k, time_):
    t.clear_canvas()
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam_at(k)
    t.options["time"] = time_
    t.render(1)


def filter_ms(t, K, ms):
    t.set_denoise(iterations=K)
    t.set_denoise_spatial_variance(ms)
    t.resolve_denoised(1)
    out = t.last_kernel_ms()[1]
    assert t.last_filter_spatial_variance() == (ms > 0 and K >= 1)
    return out


def timed(t, reps):
    rounds = {(K, ms): [] for K in (1, 5) for ms in (0, MIN_SAMPLES)}
    for r in range(reps + 1):
        for key in rounds:
            v = filter_ms(t, *key)
            if r:
                rounds[key].append(v)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return {"filter_k5_off_ms": med[(5, 0)], "filter_k5_on_ms": med[(5, MIN_SAMPLES)], "filter_k1_off_ms": med[(1, 0)],
            "filter_k1_on_ms": med[(1, MIN_SAMPLES)], "estimate_ms": med[(5, MIN_SAMPLES)] - med[(5, 0)],
            "estimate_k1_ms": med[(1, MIN_SAMPLES)] - med[(1, 0)], "pass_ms": (med[(5, 0)] - med[(1, 0)]) / 4,
            "rounds_k5_off_ms": rounds[(5, 0)], "rounds_k5_on_ms": rounds[(5, MIN_SAMPLES)]}


def tiles_without(q):
    """the share of 16x16 tiles of the mask q (h, w) with no pixel set"""
    h, w = q.shape
    th, tw = (h + 15) // 16, (w + 15) // 16
    pad = np.zeros((th * 16, tw * 16), bool)
    pad[:h, :w] = q
    return float(1.0 - pad.reshape(th, 16, tw, 16).any(axis=(1, 3)).mean())


def probe_time(w, h, reps, lib, frames=8):
    res = {}
    t = handle(w, h, 2, "spheres", 0, lib)
    t.set_denoise()
    t.trace()
    r = timed(t, reps)
    inp = t.read_denoise_inputs()
    r["early_out_tiles"] = tiles_without((inp["albedo_hits"][..., 3] > 0) & (inp["P"] < MIN_SAMPLES))
    res["first_frame"] = r
    t.close()
    t = handle(w, h, 2, "spheres", 0, lib)
    t.set_denoise()
    t.set_denoise_temporal()
    for k in range(frames):
        next_frame(t, k, 900 + k)
    r = timed(t, reps)
    t.clear_canvas()
    hist = t.read_denoise_history()
    q = (hist["count"] < MIN_SAMPLES) & (hist["guide"][..., 1, 3] > 0)
    r["early_out_tiles"] = tiles_without(q)
    r["qualifying_pixels"] = float(q.mean())
    res["eighth_frame_temporal"] = r
    t.close()
    return res


def tone(x):
    a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    x = np.asarray(x, np.float64)
    return np.sqrt(np.clip((x * (x * a + b)) / (x * (x * c + d) + e), 0, 1))


def quality(frames=8):
    w, h = 160, 90
    res = {"min_samples": MIN_SAMPLES, "width": w, "height": h}
    for name, accel in (("spheres", 0), ("meshes", 1)):
        r = {}
        g = handle(w, h, 4096, name, accel, time_=4242)
        g.set_denoise()
        g.render(1)
        ref = tone(g.read_canvas()[..., :3])
        g.close()
        mse = []
        for ms in (0, MIN_SAMPLES):
            t = handle(w, h, 2, name, accel, time_=31)
            t.set_denoise()
            t.set_denoise_spatial_variance(ms)
            t.render(1)
            mse.append(float(np.mean((tone(t.read_denoised()[..., :3]) - ref) ** 2)))
            t.close()
        r["first_frame"] = {"mse_off": mse[0], "mse_on": mse[1], "ratio": mse[1] / mse[0]}
        g = handle(w, h, 4096, name, accel, time_=4242)
        g.options["camera_to_world"] = cam_at(frames - 1)
        g.render(1)
        ref = tone(g.read_canvas()[..., :3])
        g.close()
        outs = []
        for ms in (0, MIN_SAMPLES):
            t = handle(w, h, 2, name, accel, time_=777)
            t.set_denoise()
            t.set_denoise_temporal()
            t.set_denoise_spatial_variance(ms)
            for k in range(frames):
                next_frame(t, k, 900 + k)
            outs.append(tone(t.read_denoised()[..., :3]))
            t.clear_canvas()
            hist = t.read_denoise_history()
            t.close()
        dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)  # a first hit, and no history reached it
        m = [float(np.mean((o - ref) ** 2)) for o in outs]
        md = [float(np.mean((o[dis] - ref[dis]) ** 2)) for o in outs]
        r["eighth_frame_moving"] = {"mse_off": m[0], "mse_on": m[1], "ratio": m[1] / m[0], "no_history_fraction": float(dis.mean()),
                                    "no_history_mse_off": md[0], "no_history_mse_on": md[1], "no_history_ratio": md[1] / md[0]}
        res[name] = r
        print(name, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--build-only", action="store_true", help="build the library and the global-load variant, measure nothing")
    a = ap.parse_args()
    B.build_hip()
    if not GLOBAL_LIB.exists() or GLOBAL_LIB.stat().st_mtime < B.LIB.stat().st_mtime:
        B.build_variant("sv_global", ["-DSRT_SV_GLOBAL"])
    if a.build_only:
        return
    libs = {"lds": None, "global": TR._bind(C.CDLL(str(GLOBAL_LIB)))}
    out = Path(a.out_dir) if a.out_dir else None
    if out:
        out.mkdir(parents=True, exist_ok=True)
    for s in a.sizes.split(","):
        w, h = (int(v) for v in s.split("x"))
        t0 = time.time()
        res = {"width": w, "height": h, "reps": a.reps, "min_samples": MIN_SAMPLES, "scene": "spheres", "spp": 2}
        for form, lib in libs.items():
            res[form] = probe_time(w, h, a.reps, lib)
            print(f"{w}x{h}", form, json.dumps({k: {kk: vv for kk, vv in v.items() if not kk.startswith("rounds_")} for k, v in res[form].items()}), flush=True)
        res["wall_s"] = round(time.time() - t0, 1)
        if out:
            (out / f"r18_spatial_variance_{w}x{h}.json").write_text(json.dumps(res, indent=1))
    if not a.no_quality:
        q = quality()
        if out:
            (out / "r18_spatial_variance_quality.json").write_text(json.dumps(q, indent=1))


if __name__ == "__main__":
    main()
