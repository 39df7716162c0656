"""Device time of the denoiser's stages (srt_set_denoise) at 960x540 and 1920x1080, from the library's own HIP events:

  trace_off / trace_on     srt_trace (trace kernel + ordered reduction; with the denoiser also the feature pass and the
                           moments reduction) at `spp`, denoiser off / on (feature_samples = 1)
  kernel_off / kernel_on   the trace kernel alone (srt_last_trace_kernel_ms)
  reduce_plain / reduce_moments_plus_features   trace - kernel, off / on
  feature_per_sample       trace_on(feature_samples = 2) - trace_on(feature_samples = 1): one more primary ray per pixel
  filter[K]                srt_resolve_denoised with K = 0..8 passes (set-up + K passes + tonemap); pass k = filter[k+1] - filter[k]

Medians over --reps dispatches. Scenes: the sphere scene and the two-mesh scene (array scan and BVH).
Writes one JSON per size to --out-dir (profiles/r05_denoise_<w>x<h>.json).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import build as B, records as R, scenes as S, tracer as TR  # noqa: E402


def handle(w, h, spp, name, accel):
    shapes, tris, mats = S.sphere_scene() if name == "spheres" else S.mesh_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t


def trace_ms(t, reps):
    tr, k = [], []
    for i in range(reps):
        t.options["time"] = 1000 + i
        t.trace()
        a, _ = t.last_kernel_ms()
        tr.append(a)
        k.append(t.last_trace_kernel_ms())
    return statistics.median(tr[1:]), statistics.median(k[1:])


def filter_ms(t, K, reps):
    t.set_denoise(iterations=K)  # (same feature_samples: no clear)
    out = []
    for _ in range(reps):
        t.resolve_denoised(1)
        out.append(t.last_kernel_ms()[1])
    return statistics.median(out[1:])


def probe(w, h, spp, reps):
    res = {"width": w, "height": h, "spp": spp, "reps": reps, "scenes": {}}
    for name, accel in (("spheres", 0), ("meshes", 0), ("meshes", 1)):
        key = f"{name}{'_bvh' if accel else ''}"
        t = handle(w, h, spp, name, accel)
        off, k_off = trace_ms(t, reps)
        t.set_denoise(feature_samples=1)
        on, k_on = trace_ms(t, reps)
        t.set_denoise(feature_samples=2)
        on2, _ = trace_ms(t, reps)
        t.set_denoise(feature_samples=1)
        trace_ms(t, 2)
        r = {"trace_off_ms": off, "trace_on_ms": on, "kernel_off_ms": k_off, "kernel_on_ms": k_on,
             "reduce_plain_ms": off - k_off, "reduce_moments_plus_features_ms": on - k_on,
             "feature_per_sample_ms": on2 - on, "trace_per_sample_ms": k_off / spp}
        if name == "spheres":
            f = {K: filter_ms(t, K, reps) for K in range(0, 9)}
            r["filter_ms"] = f
            r["pass_ms"] = {k: f[k + 1] - f[k] for k in range(8)}
        t.close()
        res["scenes"][key] = r
        print(key, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    B.build_hip()
    for s in a.sizes.split(","):
        w, h = (int(v) for v in s.split("x"))
        t0 = time.time()
        res = probe(w, h, a.spp, a.reps)
        res["wall_s"] = round(time.time() - t0, 1)
        if a.out_dir:
            p = Path(a.out_dir) / f"r05_denoise_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
