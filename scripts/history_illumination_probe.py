"""Device time of the moved-camera temporal set-up with the history reprojected as colour and as illumination
(srt_set_denoise_history_illumination), and the quality of a moving camera over a textured scene with the switch off and on.

  setup_colour_ms        srt_resolve_denoised with K = 0, temporal on, the camera moved since the history, the switch off:
                         srt_temporal_kernel<0, false, false>, the launch of a library without the switch (library HIP events)
  setup_illumination_ms  the same frame with the switch on: srt_temporal_kernel<0, true, false>
  ratio                  setup_illumination_ms / setup_colour_ms

Switch off and on alternate in one process on one handle and one canvas; medians of --reps rounds (default 7) after one round
that is thrown away. Scene: scenes.textured_noise_scene, 2 spp, 2 feature samples. Writes profiles/r19_history_illumination_<w>x<h>.json
to --out-dir. --quality adds profiles/r19_history_illumination_quality.json: the tonemapped MSE of the last of 8 moving frames at
2 spp (160x90) against a 4096-spp image at its camera, switch on over switch off -- the noise-textured scene under demodulation
and K = 5, and the untextured sphere and mesh scenes of scripts/temporal_probe.py --quality with the default denoiser (with their
ratio against the spatial filter alone, whole frame and on the pixels no history reached).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import build as B, records as R, scenes as S, tracer as TR  # noqa: E402


def handle(w, h, spp, name, accel=0):
    textures = bindings = None
    if name == "noise":
        shapes, tris, mats, textures, bindings = S.textured_noise_scene()
    else:
        shapes, tris, mats = S.sphere_scene() if name == "spheres" else S.mesh_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    if textures is not None:
        t.set_textures(textures)
        t.set_material_textures(bindings)
    t.clear_canvas()
    t.scene = (shapes, tris, mats)
    return t


def cam_at(k):
    return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)


def probe(w, h, reps):
    t = handle(w, h, 2, "noise")
    t.set_denoise(iterations=0, feature_samples=2)
    t.set_denoise_temporal()
    t.trace()
    t.clear_canvas()  # the history, at the default camera
    t.options["camera_to_world"] = cam_at(1)
    t.options["time"] = 1235
    t.trace()
    ms = {False: [], True: []}
    for rep in range(reps + 1):
        for on in (False, True):
            t.set_denoise_history_illumination(on)
            t.resolve_denoised(1)
            v = t.last_kernel_ms()[1]
            assert t.last_setup_history_illumination() == on
            if rep:
                ms[on].append(v)
    r = {"width": w, "height": h, "spp": 2, "reps": reps, "scene": "textured_noise_scene",
         "setup_colour_ms": statistics.median(ms[False]), "setup_illumination_ms": statistics.median(ms[True]),
         "setup_colour_ms_all": ms[False], "setup_illumination_ms_all": ms[True]}
    r["ratio"] = r["setup_illumination_ms"] / r["setup_colour_ms"]
    t.close()
    return r


def tone(x):
    a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    x = np.asarray(x, np.float64)
    return np.sqrt(np.clip((x * (x * a + b)) / (x * (x * c + d) + e), 0, 1))


def quality(frames=8):
    w, h = 160, 90
    res = {}
    for name, accel in (("noise", 0), ("spheres", 0), ("meshes", 1)):
        textured = name == "noise"
        g = handle(w, h, 4096, name, accel)
        g.options["camera_to_world"] = cam_at(frames - 1)
        g.options["time"] = 4242
        g.render(1)
        ref = tone(g.read_canvas()[..., :3])
        g.close()
        runs = {}
        for mode in ("spatial", "off", "on"):
            t = handle(w, h, 2, name, accel)
            if textured:  # the guide's texel is the canvas's; the passes filter illumination
                t.set_denoise(iterations=5, feature_samples=2)
                t.set_denoise_demodulation(True)
            else:
                t.set_denoise()
            if mode != "spatial":
                t.set_denoise_temporal()
                t.set_denoise_history_illumination(mode == "on")
            for k in range(frames):
                t.clear_canvas()
                t.update_scene(*t.scene)
                t.options["camera_to_world"] = cam_at(k)
                t.options["time"] = 900 + k
                t.render(1)
            out = tone(t.read_denoised()[..., :3])
            dis = None
            if mode == "on":
                t.clear_canvas()
                hist = t.read_denoise_history()
                dis = (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0)  # a first hit, and no history reached it
            runs[mode] = (out, dis)
            t.close()
        mse = lambda x, m=slice(None): float(np.mean((x[m] - ref[m]) ** 2))
        dis = runs["on"][1]
        sp, off, on = (runs[m][0] for m in ("spatial", "off", "on"))
        res[name] = {"spatial_mse": mse(sp), "off_mse": mse(off), "on_mse": mse(on), "ratio": mse(on) / mse(off),
                     "on_over_spatial": mse(on) / mse(sp), "disoccluded_fraction": float(dis.mean()),
                     "disoccluded_on_over_spatial": mse(on, dis) / mse(sp, dis)}
        print(name, json.dumps(res[name]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    B.build_hip()
    for s in a.sizes.split(","):
        if not s:
            continue
        w, h = (int(v) for v in s.split("x"))
        res = probe(w, h, a.reps)
        print(json.dumps(res), flush=True)
        if a.out_dir:
            p = Path(a.out_dir) / f"r19_history_illumination_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))
    if a.quality:
        q = quality()
        if a.out_dir:
            p = Path(a.out_dir) / "r19_history_illumination_quality.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(q, indent=1))


if __name__ == "__main__":
    main()
