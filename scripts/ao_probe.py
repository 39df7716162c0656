"""What the ambient-occlusion pass costs (include/srt_abi.h "ambient-occlusion pass"). One JSON document:

  rows      per scene (the bench sphere scene, the two 968-triangle meshes, the 99,904-triangle mesh, hierarchies under `sah`),
            frame (960x540, 1920x1080) and sample count (4, 16, 64), taking turns REPS times after one warm-up round:
              pass_ms      srt_render_ao under the kernel timers (srt_last_ray_query_ms: the surface kernel and the ray kernel)
              view_ms      srt_resolve_ao_view under the same timers
              pass_wall_ms srt_render_ao from an idle stream to srt_synchronize, on the host's clock
            and the parent's pieces over the very rays srt_ao_rays emits (uploaded once, outside the timing):
              ids_wall_ms  srt_render_ids, host's clock as above (the ID pass takes no timer events)
              occlusion_ms srt_occluded_rays_device under the kernel timers
            pass_over_pieces = pass_ms / (ids_wall_ms + occlusion_ms). ids_wall_ms holds a launch's host overhead, which pass_ms
            does not: pass_wall_over_pieces_wall puts both sides on the host's clock. Rows of more than MAX_RAYS rays measure
            the pass alone (their rays would not fit a sensible staging buffer). The counts are compared on the way.
  frames    per scene at 960x540: an AO viewport frame (pass + view + read-back of the bytes) beside a 2-spp path-traced frame
            (srt_render), host's clock, medians of FRAMES.
  loop      with --parent-lib PATH (a build of the parent commit): the pipelined 960x540 loop of scripts/ray_query_probe.py
            without any pass, this library and the parent's in turn, each run a process of its own; medians and both spreads.

    python scripts/ao_probe.py [--parent-lib PATH] [--out FILE] [--quick]
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
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

REPS = 5
FRAMES = 40
MAX_RAYS = 40_000_000


def med(xs):
    return float(statistics.median(xs))


def wall(t, fn):
    t.synchronize()
    t0 = time.perf_counter()
    fn()
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rows_and_frames(quick):
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S, tracer as T
    scenes = [("spheres", S.sphere_scene(), 0), ("mesh2_bvh", S.mesh_scene(), 1), ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)]
    sizes = [(960, 540)] if quick else [(960, 540), (1920, 1080)]
    cam, sky, dev = S.default_camera(), S.synthetic_sky(), torch.device("cuda", 0)
    rows, frames = [], []
    for name, (shapes, tris, mats), accel in scenes:
        for w, h in sizes:
            t = T.Tracer(w, h)
            t.set_skybox(sky)
            t.set_acceleration(accel)
            t.options = R.render_data(w, h, 2, 10, camera_to_world=cam)
            t.scene_data = R.scene_data(len(shapes))
            t.update_scene(shapes, tris, mats)
            t.set_kernel_timers(True)
            for s in (4, 16, 64):
                n = w * h * s
                pieces = n <= MAX_RAYS
                ms = {k: [] for k in ("pass_ms", "view_ms", "pass_wall_ms", "ids_wall_ms", "occlusion_ms", "occlusion_wall_ms")}
                if pieces:
                    rays = t.ao_rays(samples=s)
                    rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8)).to(dev)
                    occ_dev = torch.zeros(((n + 63) // 64,), dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    del rays
                for rep in range(REPS + 1):  # the first warms up; in turn, so that drift lands on all of them
                    ms["pass_wall_ms"].append(wall(t, lambda: t.render_ao(samples=s)))
                    ms["pass_ms"].append(t.last_ray_query_ms())
                    t.resolve_ao_view()
                    ms["view_ms"].append(t.last_ray_query_ms())
                    if pieces:
                        ms["ids_wall_ms"].append(wall(t, t.render_ids))
                        ms["occlusion_wall_ms"].append(wall(t, lambda: t.occluded_rays_device(rays_dev.data_ptr(), n, occ_dev.data_ptr(), unit=True)))
                        ms["occlusion_ms"].append(t.last_ray_query_ms())
                occ, _ = t.read_ao()
                surf = occ != 0xFFFFFFFF
                row = {"scene": name, "size": f"{w}x{h}", "samples": s, "rays": n, "surfaces": int(surf.sum()),
                       "mean_occluded": round(float(occ[surf].mean() / s), 4) if surf.any() else None}
                if pieces:
                    bits = R.mask_bits(occ_dev.cpu().numpy().view(np.uint64), n).reshape(w * h, s).sum(axis=1)
                    assert np.array_equal(bits[surf.ravel()], occ[surf]), (name, w, h, s)
                    del rays_dev, occ_dev
                for k, v in ms.items():
                    if v:
                        row[k] = round(med(v[1:]), 4)
                        row[k + "_min_max"] = [round(min(v[1:]), 4), round(max(v[1:]), 4)]
                if pieces:
                    row["pass_over_pieces"] = round(row["pass_ms"] / (row["ids_wall_ms"] + row["occlusion_ms"]), 3)
                    row["pass_wall_over_pieces_wall"] = round(row["pass_wall_ms"] / (row["ids_wall_ms"] + row["occlusion_wall_ms"]), 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
            if (w, h) == (960, 540):
                out = np.zeros(w * h * 4, np.uint8)
                ao, traced = [], []
                for k in range(FRAMES):
                    t0 = time.perf_counter()
                    t.render_ao(samples=16)
                    t.resolve_ao_view()
                    t.read_argb()
                    ao.append((time.perf_counter() - t0) * 1e3)
                    t.clear_canvas()
                    t.synchronize()
                    t0 = time.perf_counter()
                    t.render(1, out)
                    traced.append((time.perf_counter() - t0) * 1e3)
                frames.append({"scene": name, "size": f"{w}x{h}", "ao_16_frame_ms": round(med(ao[8:]), 4), "traced_2spp_frame_ms": round(med(traced[8:]), 4),
                               "ao_over_traced": round(med(ao[8:]) / med(traced[8:]), 3)})
                print(json.dumps(frames[-1]), flush=True)
            t.close()
    return rows, frames


def loop(parent_lib):
    runs = {"this": [], "parent": []}
    for rep in range(REPS):
        for name, lib in (("this", None), ("parent", parent_lib)):  # in turn, so that drift of the machine lands on both
            env = dict(os.environ)
            env.pop("SRT_LIB", None)
            if lib:
                env["SRT_LIB"] = str(lib)
            r = subprocess.run([sys.executable, str(ROOT / "scripts" / "ray_query_probe.py"), "--loop-child", "0"], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"{name}: the loop failed ({r.returncode}):\n{r.stdout}{r.stderr}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_frame"])
    res = {name: {"ms_per_frame_median": round(med(v), 4), "runs": [round(x, 4) for x in v]} for name, v in runs.items()}
    res["this_over_parent"] = round(med(runs["this"]) / med(runs["parent"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit, for the loop without the pass")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="960x540 only")
    a = ap.parse_args()
    rows, frames = rows_and_frames(a.quick)
    doc = {"reps": REPS, "rows": rows, "frames": frames}
    if a.parent_lib:
        doc["loop"] = loop(a.parent_lib)
        print(json.dumps({"loop": doc["loop"]}), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
