"""Cost of bloom for the resolve (srt_set_bloom).

resolve (--sizes, default 960x540 and 1920x1080; a planted canvas of log-uniform luminances over 2^-6 .. 2^10, no trace):
  srt_resolve between the library's resolve events (srt_last_kernel_ms), medians of --reps calls after --warmup, the modes
  taking turns call by call on one handle, MANUAL exposure on in all of them:
    exposed_ms    bloom off: srt_resolve_kernel and srt_exposure_resolve_kernel
    bloom<N>_ms   bloom with levels = N (1, 4, 6, 8) at the defaults otherwise: the plain resolve, N reduces, N - 1
                  expand-and-adds and the composite, 2 N launches in place of the exposed resolve's one
pipelined (960x540, 2 spp, scenes.sphere_scene): frames per second of the two-deep srt_render_pipelined loop on the host clock
  from the first enqueue to the flush, --frames frames after --warmup-frames, MANUAL exposure with bloom off and with bloom at
  its defaults in turn, --rounds rounds, medians.
With a library that lacks the feature (SRT_LIB: a parent checkout's build) only exposed_ms and the off rate are reported, under
--tag. --no-pipelined leaves the loop out (a run under a profiler). Writes profiles/r26_bloom_<tag>.json to --out-dir.
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
from simple_raytracer_amd import records as R, scenes as S, tracer as TR  # noqa: E402

F32 = np.float32
LEVELS = (1, 4, 6, 8)


def frame(n):
    rng = np.random.RandomState(5)
    px = np.ones((n, 4), F32)
    px[:, :3] = (np.exp2(rng.uniform(-6, 10, n))[:, None] * rng.uniform(0.2, 3.0, (n, 3))).astype(F32)
    return px


def set_mode(t, mode):
    if mode == "exposed":
        t.set_bloom(False)
    else:
        t.set_bloom(levels=int(mode[len("bloom"):]))


def resolve_cost(w, h, reps, warmup, modes):
    import torch
    t = TR.Tracer(w, h)
    t.set_exposure(mode="manual", ev=-2.0)
    c = torch.from_numpy(frame(w * h).reshape(h, w, 4)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    t.bind_canvas(c.data_ptr(), c.numel() * 4)
    ms = {m: [] for m in modes}
    for rep in range(warmup + reps):
        for m in modes:
            if len(modes) > 1:
                set_mode(t, m)
            t.resolve(1)
            if rep >= warmup:
                ms[m].append(t.last_kernel_ms()[1])
    out = {f"{m}_ms": statistics.median(v) for m, v in ms.items()}
    out.update({f"{m}_ms_p10_p90": [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for m, v in ms.items()})
    t.bind_canvas(0, 0)
    t.close()
    return out


def pipelined_rate(frames, warmup, rounds, modes):
    w, h, spp = 960, 540, 2
    shapes, tris, mats = S.sphere_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.set_exposure(mode="manual", ev=3.0)
    buf = np.zeros(w * h * 4, np.uint8)
    fps = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            if len(modes) > 1:
                t.set_bloom(m == "bloom")
            for k in range(warmup):
                t.render_pipelined(k + 1, buf)
            t.pipeline_flush(buf)
            t.synchronize()
            t0 = time.perf_counter()
            for k in range(frames):
                t.render_pipelined(k + 1, buf)
            t.pipeline_flush(buf)
            t.synchronize()
            fps[m].append(frames / (time.perf_counter() - t0))
    t.close()
    return {"size": [w, h], "spp": spp, "frames": frames, **{f"{m}_fps": statistics.median(v) for m, v in fps.items()},
            **{f"{m}_fps_all": v for m, v in fps.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--warmup-frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-pipelined", action="store_true")
    ap.add_argument("--tag", default="cost")
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():  # (torch holds the planted canvas: its runtime starts before the library's, as under pytest)
        raise SystemExit("no HIP device")
    torch.cuda.init()
    has = hasattr(TR.load_library(), "srt_set_bloom")
    res = {"library": TR.load_library().srt_version().decode(), "has_bloom": has, "reps": a.reps, "resolve": {}}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        res["resolve"][size] = resolve_cost(w, h, a.reps, a.warmup, ["exposed"] + [f"bloom{n}" for n in LEVELS] if has else ["exposed"])
    if not a.no_pipelined:
        res["pipelined"] = pipelined_rate(a.frames, a.warmup_frames, a.rounds, ["off", "bloom"] if has else ["off"])
    out = Path(a.out_dir) / f"r26_bloom_{a.tag}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
