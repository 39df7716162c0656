"""What a ray query costs (include/srt_abi.h "ray queries"), next to the work it shares code with. One JSON document:

  cast            the centre rays of a 1920x1080 and a 960x540 frame of the bench sphere scene, the two-mesh scene (array scan and
                  hierarchy) and the 99,904-triangle scene (hierarchy), cast with the device form under the kernel timers
                  (srt_last_ray_query_ms), beside the denoiser's feature pass on the same handle in the same run: one more
                  feature sample per pixel, trace(feature_samples = 2) - trace(feature_samples = 1), the method of
                  scripts/denoise_probe.py. The feature pass is the same closest-hit work behind the camera set-up, with 32 B of
                  read-modify-write per pixel against 64 B in and out here.
  pick_latency    the blocking time of a one-ray srt_pick (upload, two launches, read-back) at 960x540, beside a blocking
                  srt_render of 2 spp on the same handle.
  interference    the two-deep pipelined loop at 960x540, 2 spp (scripts/interactive_probe.py), with one srt_pick every 16th
                  frame, without it, and -- with --parent-lib PATH, a build of the parent commit -- on that library; each in a
                  process of its own, REPS times in turn, medians.

    python scripts/ray_query_probe.py [--parent-lib PATH] [--out FILE] [--quick]
"""
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
import numpy as np  # noqa: E402

REPS = 5
FRAMES = 400


def med(xs):
    return float(statistics.median(xs))


def centre_rays(R, cam, w, h):
    """RAY records of the pixel centres of a w x h frame, as the kernel forms camera rays (to the last bits of the normalisation)"""
    F = np.float32
    px, py = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    ndc_x, ndc_y = (px.ravel() + F(0.5)) / F(w), (py.ravel() + F(0.5)) / F(h)
    sx = ((F(2) * ndc_x - F(1)) * (F(w) / F(h))).astype(F)
    sy = (F(1) - F(2) * ndc_y).astype(F)
    v = (cam[0, :3][None] * sx[:, None] + cam[1, :3][None] * sy[:, None]) - cam[2, :3][None]
    v = (v / np.sqrt((v * v).sum(axis=1, dtype=F))[:, None]).astype(F)
    return R.rays(cam[3, :3], v)


def cast_costs(quick):
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    scenes = [("spheres", S.sphere_scene(), 0), ("mesh2_scan", S.mesh_scene(), 0), ("mesh2_bvh", S.mesh_scene(), 1),
              ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)]
    sizes = [(960, 540)] if quick else [(1920, 1080), (960, 540)]
    cam, sky = S.default_camera(), S.synthetic_sky()
    dev = torch.device("cuda", 0)
    out = []
    for name, (shapes, tris, mats), accel in scenes:
        for w, h in sizes:
            t = Tracer(w, h)
            t.set_skybox(sky)
            t.set_acceleration(accel)
            t.options = R.render_data(w, h, 2, 10, camera_to_world=cam)
            t.scene_data = R.scene_data(len(shapes))
            t.update_scene(shapes, tris, mats)
            t.set_kernel_timers(True)
            rays = centre_rays(R, cam, w, h)
            n = len(rays)
            rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
            hits_dev = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            cast = []
            for rep in range(REPS + 1):  # the first warms up
                t.cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True)
                cast.append(t.last_ray_query_ms())
            hits = hits_dev.cpu().numpy().view(np.uint32)
            on = {}
            for fs in (1, 2):
                t.set_denoise(iterations=0, feature_samples=fs)
                ms = []
                for rep in range(REPS + 1):
                    t.clear_canvas()
                    t.trace()
                    ms.append(t.last_kernel_ms()[0])
                on[fs] = med(ms[1:])
            c, f = med(cast[1:]), on[2] - on[1]
            out.append({"scene": name, "size": f"{w}x{h}", "rays": n, "hits": int((hits[:, 7] & 1).sum()), "cast_ms": round(c, 4),
                        "cast_ns_per_ray": round(c * 1e6 / n, 3), "feature_sample_ms": round(f, 4), "feature_ns_per_ray": round(f * 1e6 / n, 3),
                        "cast_over_feature": round(c / f, 3) if f > 0 else None, "trace_fs1_ms": round(on[1], 4), "trace_fs2_ms": round(on[2], 4)})
            print(json.dumps(out[-1]), flush=True)
            t.close()
    return out


def pick_latency():
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    w, h = 960, 540
    res = {}
    for name, scn, accel in (("spheres", S.sphere_scene(), 0), ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)):
        shapes, tris, mats = scn
        t = Tracer(w, h)
        t.set_skybox(S.synthetic_sky())
        t.set_acceleration(accel)
        t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera())
        t.scene_data = R.scene_data(len(shapes))
        t.update_scene(shapes, tris, mats)
        out = np.zeros(w * h * 4, np.uint8)
        picks, renders = [], []
        for k in range(60):
            t0 = time.perf_counter()
            t.pick([[480.5 + k, 270.5]])
            picks.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            t.render(k + 1, out)
            renders.append(time.perf_counter() - t0)
        res[name] = {"pick_ms": round(med(picks[10:]) * 1e3, 4), "render_2spp_ms": round(med(renders[10:]) * 1e3, 4),
                     "pick_over_render": round(med(picks[10:]) / med(renders[10:]), 3)}
        t.close()
    return res


def loop_child(with_pick):
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
            t.render_pipelined(frame + 1, out)
            if with_pick and frame % 16 == 15:
                t.pick([[480.5, 270.5]])
        t.pipeline_flush(out)
        dt = time.perf_counter() - t0
    print(json.dumps({"ms_per_frame": dt / FRAMES * 1e3}))
    t.close()


def interference(parent_lib):
    modes = [("with_pick", None, True), ("without_pick", None, False)]
    if parent_lib:
        modes.append(("parent_library", parent_lib, False))
    runs = {m[0]: [] for m in modes}
    for rep in range(REPS):
        for name, lib, with_pick in modes:  # in turn, so that drift of the box lands on all of them
            env = dict(os.environ)
            env.pop("SRT_LIB", None)
            if lib:
                env["SRT_LIB"] = str(lib)
            r = subprocess.run([sys.executable, __file__, "--loop-child", "1" if with_pick else "0"], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"{name}: the loop failed ({r.returncode}):\n{r.stdout}{r.stderr}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_frame"])
    res = {name: {"ms_per_frame_median": round(med(v), 4), "runs": [round(x, 4) for x in v]} for name, v in runs.items()}
    res["with_over_without"] = round(med(runs["with_pick"]) / med(runs["without_pick"]), 4)
    if parent_lib:
        res["without_over_parent"] = round(med(runs["without_pick"]) / med(runs["parent_library"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit, for the interference loop")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="960x540 only")
    ap.add_argument("--loop-child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child is not None:
        loop_child(a.loop_child == "1")
        return
    doc = {"cast": cast_costs(a.quick), "pick_latency": pick_latency()}
    print(json.dumps({"pick_latency": doc["pick_latency"]}), flush=True)
    doc["interference"] = interference(a.parent_lib)
    print(json.dumps({"interference": doc["interference"]}), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
