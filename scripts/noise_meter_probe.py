"""Cost of noise metering and of render-until-converged (srt_set_noise_meter).

meter (--sizes, default 960x540 and 1920x1080): one srt_meter_noise / srt_resolve_noise_view between two events on the handle's
  stream (bound to a torch stream for the events), medians of --reps calls after --warmup, on traced frames:
    one_bin_ms  an empty scene (sky only), meant as the frame whose waves all vote one bin; the sampled sky is not that flat: its
                pixels spread over some 90 bins (one_bin_bins_in_use), so this is a second noise frame, not the vote's best case
    noise_ms    the sphere scene after 4 dispatches of 2 spp: lanes of a wave scatter over the bins
    view_ms     the same frame through srt_resolve_noise_view (the heat map's store on top)
  each is the record's clear, the kernel and the 1,060-byte copy; traffic_ms is 20 B (24 B with the view) per pixel at 6.3 TB/s.
until (960x540, 2 spp, sphere scene): wall time of srt_render_until that stops at max_dispatches = --dispatches (threshold
  2^-24, check_every 4) against a plain loop of as many srt_trace calls and one srt_resolve_denoised + read-back, taking turns,
  --rounds rounds; `plain` is what a library without the feature can run.
pipelined (960x540, 2 spp): frames per second of the two-deep srt_render_pipelined loop with the denoiser on (K = 0), the meter
  off and on at check_every 1, 4 and 16, taking turns.
estimator (160x90, sphere and mesh scenes): at T = 1, 4, 16, 64 dispatches of 2 spp the per-pixel ratio of se to the actual
  luminance error |L - L_4096| against a 4096-spp image (pixels with an error above 1e-6): median and 10 / 90 percent points;
  and the T at which the defaults (threshold 0.05) stop.
With a library that lacks the feature (SRT_LIB: a parent checkout's build) only the plain loop and the meter-off rate are
reported. Writes profiles/r27_noise_meter_<tag>.json to --out-dir.
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
sys.path.insert(0, str(ROOT / "tests"))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S, tracer as TR  # noqa: E402

F32 = np.float32


def tracer_of(w, h, scene, spp=2, time_=1234, denoise=True):
    shapes, tris, mats = scene
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=time_)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    if denoise:
        t.set_denoise(iterations=0)
    return t


def spread(v):
    return {"median": statistics.median(v), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


def meter_cost(w, h, reps, warmup):
    import torch
    stream = torch.cuda.Stream()
    shapes, tris, mats = S.sphere_scene()
    out = {"traffic_ms": w * h * 20 / 6.3e12 * 1e3, "traffic_view_ms": w * h * 24 / 6.3e12 * 1e3}
    for name, scene in (("one_bin", (np.zeros(0, R.SHAPE), tris, mats)), ("noise", (shapes, tris, mats))):
        t = tracer_of(w, h, scene)
        t.set_noise_meter()
        for k in range(4):
            t.options["time"] = np.uint32(1234 + 7919 * k)
            t.trace()
        t.synchronize()
        t.bind_stream(stream.cuda_stream)
        for what, call in (("", t.meter_noise), ("view", t.resolve_noise_view)):
            if name == "one_bin" and what:
                continue
            ms = []
            for rep in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if rep >= warmup:
                    ms.append(e0.elapsed_time(e1))
            out[(what or name) + "_ms"] = spread(ms)
        res = t.read_noise()
        out[name + "_bins_in_use"] = int(np.count_nonzero(res["hist"]))
        t.bind_stream(0)
        t.close()
    return out


def until_cost(dispatches, rounds, has):
    w, h = 960, 540
    t = tracer_of(w, h, S.sphere_scene())
    if has:
        t.set_noise_meter(threshold=2.0 ** -24, check_every=4)
        t.set_noise_meter(False)
    secs = {"plain": [], "until": []} if has else {"plain": []}
    for rnd in range(rounds + 1):
        for mode in secs:
            t.clear_canvas()
            t.synchronize()
            t0 = time.perf_counter()
            if mode == "until":
                t.set_noise_meter(threshold=2.0 ** -24, check_every=4)
                _, res, done = t.render_until(dispatches)
                assert done == dispatches and not res["converged"]
                t.set_noise_meter(False)
            else:
                for i in range(dispatches):
                    t.options["time"] = np.uint32(1234 + 7919 * i)
                    t.trace()
                t.options["time"] = np.uint32(1234)
                t.resolve_denoised(dispatches)
                t.read_argb()
            if rnd:
                secs[mode].append(time.perf_counter() - t0)
    t.close()
    return {"size": [w, h], "spp": 2, "dispatches": dispatches, **{m + "_s": spread(v) for m, v in secs.items()}, **{m + "_s_all": v for m, v in secs.items()}}


def pipelined_rate(frames, warmup, rounds, has):
    w, h = 960, 540
    t = tracer_of(w, h, S.sphere_scene())
    modes = ["off", 1, 4, 16] if has else ["off"]
    buf = np.zeros(w * h * 4, np.uint8)
    fps = {str(m): [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            if has:
                t.set_noise_meter(False) if m == "off" else t.set_noise_meter(check_every=m)
            t.clear_canvas()
            for k in range(warmup):
                t.render_pipelined(k + 1, buf)
            t.pipeline_flush(buf)
            t.synchronize()
            t0 = time.perf_counter()
            for k in range(frames):
                t.render_pipelined(warmup + k + 1, buf)
            t.pipeline_flush(buf)
            t.synchronize()
            fps[str(m)].append(frames / (time.perf_counter() - t0))
    t.close()
    return {"size": [w, h], "spp": 2, "frames": frames, "denoiser": "K = 0", **{f"check_every_{m}_fps": spread(v) for m, v in fps.items()},
            **{f"check_every_{m}_fps_all": v for m, v in fps.items()}}


def estimator():
    import noise_ref as N
    w, h = 160, 90
    out = {}
    for name, scene in (("spheres", S.sphere_scene()), ("meshes", S.mesh_scene())):
        t = tracer_of(w, h, scene, spp=4096, time_=99, denoise=False)
        t.trace()
        truth = N.D.lum(t.read_canvas().reshape(-1, 4)[:, :3]).astype(np.float64)
        t.close()
        t = tracer_of(w, h, scene)
        t.set_noise_meter()
        rows = {}
        for i in range(64):
            t.options["time"] = np.uint32(1234 + 7919 * i)
            t.trace()
            if i + 1 in (1, 4, 16, 64):
                inputs = t.read_denoise_inputs()
                T_, P = inputs["T"], inputs["P"]
                c, mo = t.read_canvas().reshape(-1, 4), inputs["moments"].reshape(-1)
                L = N.D.lum((c[:, :3] / F32(T_)).astype(F32)).astype(np.float64)
                v = np.maximum(mo.astype(np.float64) / T_ - L * L, 0)
                se, err = np.sqrt(v / P), np.abs(L - truth)
                ok = (err > 1e-6) & np.isfinite(se)
                ratio = se[ok] / err[ok]
                t.meter_noise()
                res = t.read_noise()
                rows[str(i + 1)] = {"pixels": int(ok.sum()), "se_over_error": spread(ratio.tolist()), "zero_se_share": float(np.mean(se[ok] == 0)),
                                    "level": float(res["level"]), "below_share": res["below"] / max(res["metered"], 1)}
        t.clear_canvas()
        t.options["time"] = np.uint32(1234)
        _, res, done = t.render_until(4096)
        out[name] = {"by_dispatches": rows, "until_noise_0.05": {"converged": res["converged"], "T_star": res["dispatches"], "dispatches_done": done,
                                                                   "level": float(res["level"])}}
        t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dispatches", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--warmup-frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-estimator", action="store_true")
    ap.add_argument("--tag", default="cost")
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():  # (torch holds the events' stream: its runtime starts before the library's, as under pytest)
        raise SystemExit("no HIP device")
    torch.cuda.init()
    has = hasattr(TR.load_library(), "srt_set_noise_meter")
    res = {"library": TR.load_library().srt_version().decode(), "has_noise_meter": has, "reps": a.reps}
    if has:
        res["meter"] = {}
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            res["meter"][size] = meter_cost(w, h, a.reps, a.warmup)
    res["until"] = until_cost(a.dispatches, a.rounds, has)
    res["pipelined"] = pipelined_rate(a.frames, a.warmup_frames, a.rounds, has)
    if has and not a.skip_estimator:
        res["estimator"] = estimator()
    out = Path(a.out_dir) / f"r27_noise_meter_{a.tag}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
