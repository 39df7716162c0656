#!/usr/bin/env python3
"""What area selection costs (csrc/area.hip), on the device:

  coverage   the blocking srt_area_coverage call (wall clock, the planes current) and its clear + launches alone (srt_last_area_ms)
             at 960x540 and 1920x1080 on the bench sphere scene: a full-frame rectangle, a 10 % rectangle, a 256-vertex lasso;
             beside each what a front-end does without the feature: read_id_pass plus numpy.bincount over the same mask
  triangles  triangle coverage of the 99,904-triangle mesh (the many-keys case) with the aggregation's round limit at 0, 2, 4 and
             8 (the development library reads SRT_AREA_ROUNDS)
  loop       the two-deep pipelined loop at 960x540, 2 spp: the feature unused (against --parent-lib, a library built from the
             parent commit), and with one select_area every 16th frame

Every measurement is the median of REPS; the runs and their spread are kept beside it. The loop's runs are processes of their
own, each under a time limit, taken in turn. One JSON document on stdout (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402

REPS = 7
FRAMES = 400
CHILD_LIMIT = 120  # seconds per child process


def med(xs):
    return float(statistics.median(xs))


def stats(xs):
    return {"median_ms": round(med(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def zigzag(w, h):
    """256 vertices: a saw over the upper half of the frame, closed along the bottom"""
    xs = np.round(np.linspace(w // 16, w - w // 16, 254)).astype(int)
    return [(int(x), h // 8 if i % 2 == 0 else h // 2) for i, x in enumerate(xs)] + [(w - w // 16, h - h // 8), (w // 16, h - h // 8)]


def handle(R, S, Tracer, scn, accel, w, h, lib=None):
    shapes, tris, mats = scn
    t = Tracer(w, h, lib=lib)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, 1, 2, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.set_kernel_timers(True)
    return t


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def coverage_costs(sizes):
    import area_ref as AR
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    doc = {}
    for (w, h) in sizes:
        t = handle(R, S, Tracer, S.sphere_scene(), 0, w, h)
        n = len(S.sphere_scene()[0])
        t.area_coverage((0, 0, w, h))  # makes the planes
        side = 10 ** -0.5
        cases = {"full_frame": ((0, 0, w, h), None), "rect_10_percent": ((w // 4, h // 4, w // 4 + int(w * side), h // 4 + int(h * side)), None),
                 "lasso_256": ((0, 0, w, h), zigzag(w, h))}
        for name, (rect, lasso) in cases.items():
            mask = AR.mask(rect, lasso, w, h)  # (the front-end's mask is its own business: not timed)
            calls, kernels, fronts = [], [], []
            for rep in range(REPS + 1):
                ms, (counts, s) = timed(lambda: t.area_coverage(rect, lasso, options=False))
                k = t.last_area_ms()

                def front_end():
                    ids = t.read_id_pass()["shape"]
                    keys = ids[mask & (ids != R.HIT_NONE)]
                    return np.bincount(keys, minlength=n)
                fms, want = timed(front_end)
                assert np.array_equal(want[:n].astype(np.uint32), counts), name
                if rep:  # the first pass warms up
                    calls.append(ms), kernels.append(k), fronts.append(fms)
            spread = max(max(calls) - min(calls), max(fronts) - min(fronts))
            gain = med(fronts) - med(calls)
            doc[f"{w}x{h} {name}"] = {"area_pixels": s["area_pixels"], "distinct": s["distinct"], "call": stats(calls), "launches": stats(kernels),
                                      "read_id_pass_plus_bincount": stats(fronts), "front_end_over_call": round(med(fronts) / med(calls), 2),
                                      "claim": "faster" if gain > spread else "no claim"}
        t.close()
    return doc


def triangle_costs(sizes):
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S, tracer as T
    dev = T.load_dev_library()
    doc = {}
    scn = S.mesh_scene(1, 224, 224)
    n_tri = int(scn[0]["num_triangles"][1])
    for (w, h) in sizes:
        t = handle(R, S, T.Tracer, scn, 1, w, h, lib=dev)
        t.options["camera_to_world"] = R.camera_matrix((0.0, 0.3, 2.2), 0.0, 0.0)  # the mesh fills most of the frame
        base = None
        for rounds in (0, 2, 4, 8):
            os.environ["SRT_AREA_ROUNDS"] = str(rounds)
            t.area_triangle_coverage(1, n_tri, (0, 0, w, h))
            calls, kernels = [], []
            for rep in range(REPS):
                ms, (counts, s) = timed(lambda: t.area_triangle_coverage(1, n_tri, (0, 0, w, h), options=False))
                calls.append(ms), kernels.append(t.last_area_ms())
            base = counts if base is None else base
            assert np.array_equal(counts, base), rounds
            doc[f"{w}x{h} rounds {rounds}"] = {"target_pixels": s["target_pixels"], "distinct": s["distinct"], "call": stats(calls), "launches": stats(kernels)}
        os.environ.pop("SRT_AREA_ROUNDS", None)
        t.close()
    return doc


def loop_child(mode):
    """one run of the pipelined loop (a process of its own: the library is whatever SRT_LIB names); prints ms per frame"""
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    w, h, spp = 960, 540, 2
    shapes, tris, mats = S.sphere_scene()
    t = Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    out = np.zeros(w * h * 4, np.uint8)
    for rep in range(2):  # the first pass warms up
        t.clear_canvas()
        t.synchronize()
        t0 = time.perf_counter()
        for frame in range(FRAMES):
            t.options["time"] = np.uint32(1000 + frame)
            if mode == "select" and frame % 16 == 0:
                x = 100 + frame
                t.select_area((x, 100, x + 300, 400))  # a marquee that moves with the drag
            t.render_pipelined(frame + 1, out)
        t.pipeline_flush(out)
        dt = time.perf_counter() - t0
    print(json.dumps({"ms_per_frame": dt / FRAMES * 1e3}))
    t.close()


def loop(parent_lib):
    modes = [("unused", None), ("select_every_16th", None)]
    if parent_lib:
        modes.insert(1, ("parent_library", parent_lib))
    runs = {m[0]: [] for m in modes}
    for rep in range(5):
        for name, lib in modes:  # in turn, so that drift of the box lands on all of them
            env = dict(os.environ)
            env.pop("SRT_LIB", None)
            if lib:
                env["SRT_LIB"] = str(lib)
            child = "select" if name == "select_every_16th" else "unused"
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, __file__, "--loop-child", child], env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started behind a failed run
                raise SystemExit(f"{name}: the loop failed ({r.returncode}):\n{r.stdout}{r.stderr}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_frame"])
    res = {name: {"ms_per_frame_median": round(med(v), 4), "runs": [round(x, 4) for x in v], "spread": round(max(v) - min(v), 4)} for name, v in runs.items()}
    res["select_over_unused"] = round(med(runs["select_every_16th"]) / med(runs["unused"]), 4)
    if parent_lib:
        res["unused_minus_parent_ms"] = round(med(runs["unused"]) - med(runs["parent_library"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="960x540 only, no loop")
    ap.add_argument("--loop-child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child is not None:
        loop_child(a.loop_child)
        return
    sizes = [(960, 540)] if a.quick else [(960, 540), (1920, 1080)]
    doc = {"coverage": coverage_costs(sizes), "triangles": triangle_costs(sizes)}
    if not a.quick:
        doc["loop"] = loop(a.parent_lib)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
