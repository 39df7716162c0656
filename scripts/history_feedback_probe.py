"""Cost and quality of the history feedback (srt_set_denoise_history_feedback).

cost (--sizes, default 960x540 and 1920x1080; scenes.sphere_scene, 2 spp, a history and a moved camera; plain and demodulated):
  filter_off_ms / filter_on_ms    srt_resolve_denoised with K = 5, the switch off and on (library HIP events around the filter)
  front_off_ms / front_on_ms      the same with K = 1: the set-up and pass 1 alone, so on - off is what the store costs pass 1
  clear_off_ms / clear_on_ms      srt_clear_canvas after a trace without a filter, on the host clock between two synchronises
                                  (K = 5): off runs the set-up alone, on the filter's front (up to four launches)
  Off and on alternate in one process on one handle and one canvas; medians of --reps rounds after one that is thrown away; two
  off series of one run (off_a, off_b). With a library that lacks the switch (SRT_LIB: a parent checkout's build) only the off
  figures are reported, under --tag (_parent, _parent2: two runs give the parent's own spread): the parent's filter, front and
  clear by the same probe, host path included. front at K = 1 times pass 1 as the LAST pass (under demodulation the remodulating
  kernel, with the ARGB write); the middle-pass kernel that pass 1 is at K = 5 is timed per kernel by --kernel-loop.
kernel loop (--kernel-loop WxH): nothing is timed here; 30 filters at K = 5 with the switch off and 30 with it on, plain and then
  demodulated, for a run under a kernel tracer whose per-kernel statistics tell pass 1's two forms apart by name.
quality (--quality): the set-up of test_quality_moving_camera (tests/test_gpu_denoise_temporal.py): 160x90, 8 frames at 2 spp on
  the moving camera, the default filter, tonemapped MSE against 4096 spp at the last camera; the MSE with the switch on over the
  MSE with it off, both in one run, on the whole frame and on the pixels the last frame could not reproject; spheres and meshes
  (BVH), demodulation off and on, three values of `time`. And the noise-textured scene of scripts/history_illumination_probe.py
  (scenes.textured_noise_scene: a texel per pixel; feature_samples 2, K = 5) in two modes: without demodulation, and with
  demodulation plus history illumination.
Writes profiles/r24_history_feedback_<w>x<h>.json and profiles/r24_history_feedback_quality.json to --out-dir.
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


def cam_at(k):
    return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)


def tracer(scn, w, h, spp, accel=0, time_=1234):
    textures = bindings = None
    if len(scn) == 5:
        shapes, tris, mats, textures, bindings = scn
        scn = (shapes, tris, mats)
    shapes, tris, mats = scn
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=time_)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    if textures is not None:
        t.set_textures(textures)
        t.set_material_textures(bindings)
    t.clear_canvas()
    t.scene = scn
    return t


def cost(w, h, reps, demod):
    t = tracer(S.sphere_scene(), w, h, 2)
    t.set_denoise(iterations=5)
    t.set_denoise_temporal()
    if demod:
        t.set_denoise_demodulation(True)
    t.trace()
    t.clear_canvas()  # the history, at the default camera
    t.options["camera_to_world"] = cam_at(1)
    t.options["time"] = 1235
    t.trace()
    out = {}
    has_switch = hasattr(t.lib, "srt_set_denoise_history_feedback")
    for name, K in (("filter", 5), ("front", 1)):
        t.set_denoise(iterations=K)
        ms = {"off_a": [], "on": [], "off_b": []} if has_switch else {"off_a": [], "off_b": []}
        for rep in range(reps + 1):
            for key in ms:
                if has_switch:
                    t.set_denoise_history_feedback(key == "on")
                t.resolve_denoised(1)
                v = t.last_kernel_ms()[1]
                if has_switch:
                    assert t.last_filter_history_feedback() == (key == "on")
                if rep:
                    ms[key].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.update({f"{name}_off_ms": med["off_a"], f"{name}_off_b_ms": med["off_b"], f"{name}_off_spread_ms": abs(med["off_a"] - med["off_b"]), f"{name}_all": ms})
        if has_switch:
            out.update({f"{name}_on_ms": med["on"], f"{name}_added_ms": med["on"] - med["off_a"]})
    t.set_denoise(iterations=5)
    clear = {False: [], True: []}
    for rep in range(reps + 1):
        for on in ((False, True) if has_switch else (False,)):
            if has_switch:
                t.set_denoise_history_feedback(on)
            t.clear_canvas()
            t.update_scene(*t.scene)
            t.options["time"] = 2000 + rep
            t.trace()
            t.synchronize()
            t0 = time.perf_counter()
            t.clear_canvas()
            t.synchronize()
            v = (time.perf_counter() - t0) * 1e3
            if rep:
                clear[on].append(v)
    out.update({"clear_off_ms": statistics.median(clear[False]), "clear_all": {"off": clear[False], "on": clear[True]}})
    if has_switch:
        out["clear_on_ms"] = statistics.median(clear[True])
    t.close()
    return out


def kernel_loop(w, h, n=30):
    for demod in (False, True):
        t = tracer(S.sphere_scene(), w, h, 2)
        t.set_denoise(iterations=5)
        t.set_denoise_temporal()
        if demod:
            t.set_denoise_demodulation(True)
        t.trace()
        t.clear_canvas()
        t.options["camera_to_world"] = cam_at(1)
        t.options["time"] = 1235
        t.trace()
        for on in (False, True):
            t.set_denoise_history_feedback(on)
            for _ in range(n):
                t.resolve_denoised(1)
            t.synchronize()
        t.close()


def aces(x):
    x = np.asarray(x, np.float64)
    return np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0.0, 1.0)


def tone(x):
    return np.sqrt(aces(x))


def quality(name, accel, demod, seed, illum=False):
    w, h, frames = 160, 90, 8
    textured = name == "noise"
    scn = S.textured_noise_scene() if textured else S.sphere_scene() if name == "spheres" else S.mesh_scene()
    g = tracer(scn, w, h, 4096, accel, 4242)
    g.options["camera_to_world"] = cam_at(frames - 1)
    g.render(1)
    ref = tone(g.read_canvas()[..., :3])
    g.close()
    runs = {}
    for on in (False, True):
        t = tracer(scn, w, h, 2, accel)
        if textured:  # the guide's texel is the canvas's (scripts/history_illumination_probe.py)
            t.set_denoise(iterations=5, feature_samples=2)
        else:
            t.set_denoise()
        t.set_denoise_temporal()
        if demod:
            t.set_denoise_demodulation(True)
        if illum:
            t.set_denoise_history_illumination(True)
        if on:
            t.set_denoise_history_feedback(True)
        for k in range(frames):
            t.clear_canvas()
            t.update_scene(*scn[:3])
            t.options["camera_to_world"] = cam_at(k)
            t.options["time"] = seed + k
            t.render(1)
        out = tone(t.read_denoised()[..., :3])
        t.clear_canvas()
        hist = t.read_denoise_history()
        runs[on] = (out, (hist["count"] == 2) & (hist["guide"][..., 1, 3] > 0))
        t.close()
    dis = runs[False][1]
    mse = lambda x, m=slice(None): float(np.mean((x[m] - ref[m]) ** 2))
    r = {"scene": name, "demodulation": demod, "history_illumination": illum, "time": seed, "mse_off": mse(runs[False][0]), "mse_on": mse(runs[True][0]), "disoccluded_share": float(dis.mean())}
    r["ratio"] = r["mse_on"] / r["mse_off"]
    r["disoccluded_ratio"] = mse(runs[True][0], dis) / mse(runs[False][0], dis) if dis.any() else None
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--tag", default="", help="appended to the cost files' names (a parent checkout's run: _parent)")
    ap.add_argument("--kernel-loop", default=None, metavar="WxH")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    B.build_hip()
    if a.kernel_loop:
        kernel_loop(*(int(v) for v in a.kernel_loop.split("x")))
        return
    out = Path(a.out_dir) if a.out_dir else None
    if out:
        out.mkdir(parents=True, exist_ok=True)
    for s in a.sizes.split(","):
        if not s:
            continue
        w, h = (int(v) for v in s.split("x"))
        res = {"width": w, "height": h, "spp": 2, "reps": a.reps, "scene": "sphere_scene", "plain": cost(w, h, a.reps, False), "demod": cost(w, h, a.reps, True)}
        print(json.dumps({k: ({x: y for x, y in v.items() if not x.endswith("all")} if isinstance(v, dict) else v) for k, v in res.items()}), flush=True)
        if out:
            (out / f"r24_history_feedback_{w}x{h}{a.tag}.json").write_text(json.dumps(res, indent=1))
    if a.quality:
        seeds = (900, 1900, 2900)
        rows = [quality(n, acc, d, seed) for n, acc in (("spheres", 0), ("meshes", 1)) for d in (False, True) for seed in seeds]
        rows += [quality("noise", 0, d, seed, illum=d) for d in (False, True) for seed in seeds]
        worst = {}
        for r in rows:
            key = f"{r['scene']}{'_demod' if r['demodulation'] else ''}{'_illum' if r['history_illumination'] else ''}"
            worst[key] = max(worst.get(key, 0.0), r["ratio"])
        res = {"frame": [160, 90], "spp": 2, "frames": 8, "runs": rows, "worst_ratio": worst}
        print(json.dumps(res), flush=True)
        if out:
            (out / "r24_history_feedback_quality.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
