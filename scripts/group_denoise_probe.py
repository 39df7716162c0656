"""Device time of a device group's frame with the denoiser (srt_group_set_denoise), against the parent commit's library.

One child process per (library, size, members) measures, with HIP events on the root member's stream (a torch stream bound
with srt_bind_stream; every other member's work reaches it through the collection), medians over --frames frames after
--warmup:

  group_off   clear, srt_group_trace_and_gather, srt_resolve_gathered: {gather = trace + collect (16 B/px) + unpermute, resolve}
  group_on    the same with the group's denoiser on, K = 5: {gather = trace + features + moments + collect (52 B/px) +
              unpermute of four planes, filter = srt_group_resolve_denoised}              (this commit only)
  single_off / single_on   one handle of the same size: srt_trace + srt_resolve / srt_resolve_denoised, denoiser off / on

The driver (no --child) starts fresh children, alternating --parent-lib (the parent commit's libsrt_hip.so, through SRT_LIB)
and this tree's library, --rounds times, and reports per quantity the median of the children's medians and their spread
(min, max). What the group adds to "parent group frame + parent single-handle denoiser" is
  extra = group_on.total - group_off.total(parent) - (single_on.total - single_off.total)(parent)
expected: the 3.25x larger collection plus one unpermute pass over 52 B per pixel. Members beyond the box's GPUs are
VIRTUAL devices: the collection is then device-to-device copies on one GPU, not xGMI traffic.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def child(a):
    import ctypes as C

    import numpy as np
    import torch

    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S, tracer as TR
    lib = TR.load_library()
    w, h, n = a.width, a.height, a.members
    shapes, tris, mats = S.sphere_scene()
    sky = S.synthetic_sky()
    stream = torch.cuda.Stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def setup(t):
        t.set_skybox(sky)
        t.options = R.render_data(w, h, a.spp, 10, camera_to_world=S.default_camera(), time=1234)
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        t.clear_canvas()
        return t

    def timed(frame):
        """frame(i) enqueues one frame in two parts and returns nothing; medians of the parts' and the whole's device ms"""
        parts = []
        for i in range(a.warmup + a.frames):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            frame(i, lambda k: ev[k].record(stream))
            ev[2].synchronize()
            parts.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[0].elapsed_time(ev[2])))
        parts = parts[a.warmup:]
        return [statistics.median(p[k] for p in parts) for k in range(3)]

    out = {"lib": os.environ.get("SRT_LIB", "tree"), "width": w, "height": h, "members": n, "spp": a.spp, "frames": a.frames}
    # ---- the group ----
    g = setup(TR.TracerGroup(w, h, n_devices=n, devices=None if n == 1 else [0] * n, rows_per_block=8))
    root = C.c_void_p(lib.srt_group_tracer(g._g, 0))
    assert lib.srt_bind_stream(root, sptr) == 0
    rd = R.as_records(g.options, R.RENDER_DATA)

    def group_frame(on):
        def frame(i, mark):
            rd["time"] = np.uint32(1000 + i)
            g.clear_canvas()
            mark(0)
            assert lib.srt_group_trace_and_gather(g._g, TR._ptr(rd)) == 0
            mark(1)
            assert (lib.srt_group_resolve_denoised(g._g, 1) if on else lib.srt_resolve_gathered(root, 1)) == 0
            mark(2)
        return frame

    ga, re_, tot = timed(group_frame(False))
    out["group_off"] = {"gather_ms": ga, "resolve_ms": re_, "total_ms": tot}
    if hasattr(lib, "srt_group_set_denoise"):
        g.set_denoise(iterations=5)
        ga, re_, tot = timed(group_frame(True))
        out["group_on"] = {"gather_ms": ga, "filter_ms": re_, "total_ms": tot}
        g.set_denoise_temporal()
        ga, re_, tot = timed(group_frame(True))
        out["group_on_temporal"] = {"gather_ms": ga, "filter_ms": re_, "total_ms": tot}
    lib.srt_bind_stream(root, None)
    g.close()
    # ---- one handle of the same size ----
    t = setup(TR.Tracer(w, h))
    t.bind_stream(sptr.value)

    def single_frame(on):
        def frame(i, mark):
            t.options["time"] = np.uint32(1000 + i)
            t.clear_canvas()
            mark(0)
            t.trace()
            mark(1)
            t.resolve_denoised(1) if on else t.resolve(1)
            mark(2)
        return frame

    tr, re_, tot = timed(single_frame(False))
    out["single_off"] = {"trace_ms": tr, "resolve_ms": re_, "total_ms": tot}
    t.set_denoise(iterations=5)
    tr, re_, tot = timed(single_frame(True))
    out["single_on"] = {"trace_ms": tr, "filter_ms": re_, "total_ms": tot}
    t.bind_stream(None)
    t.close()
    print("PROBE " + json.dumps(out), flush=True)


def summarise(runs):
    """runs: the children's dicts for one (library, size, members) -> per quantity {median, min, max} over the children"""
    res = {}
    for key in ("group_off", "group_on", "group_on_temporal", "single_off", "single_on"):
        if not all(key in r for r in runs):
            continue
        res[key] = {}
        for q in runs[0][key]:
            v = [r[key][q] for r in runs]
            res[key][q] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--member-counts", default="1,4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libsrt_hip.so (omit: this tree's library only)")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.frames >= 7
    result = {"spp": a.spp, "frames": a.frames, "warmup": a.warmup, "rounds": a.rounds, "iterations": 5, "configs": []}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in a.member_counts.split(",")):
            runs = {"parent": [], "this": []}
            for _ in range(a.rounds):
                for which in (["parent"] if a.parent_lib else []) + ["this"]:  # alternated: fresh process each
                    env = dict(os.environ)
                    env.pop("SRT_LIB", None)
                    if which == "parent":
                        env["SRT_LIB"] = a.parent_lib
                    cmd = [sys.executable, __file__, "--child", "--width", str(w), "--height", str(h), "--members", str(n), "--spp", str(a.spp),
                           "--frames", str(a.frames), "--warmup", str(a.warmup)]
                    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
                    if r.returncode != 0:  # nothing more is started on the device after a failure
                        sys.stderr.write(r.stdout + r.stderr)
                        raise SystemExit(f"child failed ({which}, {size}, {n} members): exit {r.returncode}")
                    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1]
                    runs[which].append(json.loads(line[6:]))
            cfg = {"width": w, "height": h, "members": n, "this": summarise(runs["this"])}
            if runs["parent"]:
                cfg["parent"] = p = summarise(runs["parent"])
                th = cfg["this"]
                med = lambda d, k: d[k]["total_ms"]["median"]  # noqa: E731
                cfg["denoiser_off_this_minus_parent_ms"] = round(med(th, "group_off") - med(p, "group_off"), 4)
                cfg["extra_over_parent_group_plus_single_denoiser_ms"] = round(
                    med(th, "group_on") - med(p, "group_off") - (med(p, "single_on") - med(p, "single_off")), 4)
            result["configs"].append(cfg)
            print(json.dumps(cfg), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
