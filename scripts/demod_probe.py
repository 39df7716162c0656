"""Device time of the denoiser's filter with and without albedo demodulation (srt_set_denoise_demodulation), from the
library's own HIP events (srt_last_kernel_ms after srt_resolve_denoised), on scenes.textured_noise_scene:

  guided_ms[K] / demod_ms[K]   set-up + K passes + tonemap; demodulated: + the demodulate launch, the passes without the albedo taps
  ratio[K]                     demod_ms[K] / guided_ms[K] of the same run
  pass_guided_ms / pass_demod_ms   (filter[5] - filter[1]) / 4: one pass of steps 2 .. 16
  demodulate_ms                demod_ms[1] - guided_ms[1] minus the one pass's difference: the extra launch

Guided and demodulated filters alternate in one process on one handle and one canvas; medians of --reps rounds (default 7)
after one round that is thrown away. Sizes 960x540 and 1920x1080, K = 1 and K = 5 (and K = 0, the set-up alone).
Writes one JSON per size to --out-dir (profiles/r10_demod_<w>x<h>.json).
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

KS = (0, 1, 5)


def handle(w, h, spp):
    shapes, tris, mats, textures, bindings = S.textured_noise_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.set_textures(textures)
    t.set_material_textures(bindings)
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.set_denoise(feature_samples=spp)
    t.trace()
    return t


def filter_ms(t, K, demod):
    t.set_denoise(iterations=K, feature_samples=int(t.options["num_samples"]))  # (same feature_samples: no clear)
    t.set_denoise_demodulation(demod)
    t.resolve_denoised(1)
    ms = t.last_kernel_ms()[1]
    assert t.last_filter_demodulated() == (demod and K >= 1)
    return ms


def probe(w, h, spp, reps):
    t = handle(w, h, spp)
    rounds = {(K, d): [] for K in KS for d in (False, True)}
    for r in range(reps + 1):
        for K in KS:
            for d in (False, True):
                ms = filter_ms(t, K, d)
                if r:
                    rounds[(K, d)].append(ms)
    t.close()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    res = {"width": w, "height": h, "spp": spp, "reps": reps, "scene": "textured_noise_scene",
           "guided_ms": {K: med[(K, False)] for K in KS}, "demod_ms": {K: med[(K, True)] for K in KS},
           "ratio": {K: med[(K, True)] / med[(K, False)] for K in KS},
           "pass_guided_ms": (med[(5, False)] - med[(1, False)]) / 4, "pass_demod_ms": (med[(5, True)] - med[(1, True)]) / 4,
           "rounds_guided_ms": {K: rounds[(K, False)] for K in KS}, "rounds_demod_ms": {K: rounds[(K, True)] for K in KS}}
    res["demodulate_ms"] = (med[(1, True)] - med[(1, False)]) - (res["pass_demod_ms"] - res["pass_guided_ms"])
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("rounds_")}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    B.build_hip()
    for s in a.sizes.split(","):
        w, h = (int(v) for v in s.split("x"))
        t0 = time.time()
        res = probe(w, h, a.spp, a.reps)
        res["wall_s"] = round(time.time() - t0, 1)
        if a.out_dir:
            p = Path(a.out_dir) / f"r10_demod_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
