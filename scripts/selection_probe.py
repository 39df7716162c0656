"""What the selection overlay costs (include/srt_abi.h "selection overlay and the ID pass"). One JSON document:

  id_pass         the ID pass's device time at 960x540 and 1920x1080 on the bench sphere scene, the two-mesh scene (array scan and
                  hierarchy) and the 99,904-triangle scene (hierarchy), beside srt_cast_rays_device of the same centre rays
                  (srt_last_ray_query_ms) -- on this library and, with --parent-lib PATH, on a build of the parent commit, each
                  in a process of its own. The pass has no timer of its own: with the kernel timers on, srt_resolve's span
                  (srt_last_kernel_ms) holds everything enqueued behind the plain resolve, so the pass is the span of the first
                  resolve after a camera change minus the span of the next one, whose planes are cached.
  outline         the outline kernel with its alpha-plane fill, the same way: the span of a resolve with the selection on and
                  cached planes minus the span with it off; four masks: nothing on screen, a small sphere, a mesh silhouette, a
                  plane that fills the frame.
  loop            the two-deep pipelined loop at 960x540, 2 spp (scripts/interactive_probe.py): selection off, selection on with
                  a still camera, on with a camera that moves every frame, and with --parent-lib the parent's library; each in a
                  process of its own, REPS times in turn; medians and every run, so that off against parent can be read against
                  the spread of the runs.

    python scripts/selection_probe.py [--parent-lib PATH] [--out FILE] [--quick]
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


def scenes(S):
    return [("spheres", S.sphere_scene(), 0), ("mesh2_scan", S.mesh_scene(), 0), ("mesh2_bvh", S.mesh_scene(), 1),
            ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)]


def handle(R, S, Tracer, scn, accel, w, h, spp=1):
    shapes, tris, mats = scn
    t = Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, 2, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.set_kernel_timers(True)
    return t


def resolve_ms(t):
    t.resolve(1)
    return t.last_kernel_ms()[1]


def cast_child(quick):
    """srt_cast_rays_device of the centre rays per scene and size on the library SRT_LIB names (a process of its own)"""
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    dev = torch.device("cuda", 0)
    out = {}
    for name, scn, accel in scenes(S):
        for w, h in ([(960, 540)] if quick else [(960, 540), (1920, 1080)]):
            t = handle(R, S, Tracer, scn, accel, w, h)
            rays = centre_rays(R, S.default_camera(), w, h)
            n = len(rays)
            rays_dev = torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev)
            hits_dev = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ms = []
            for rep in range(REPS + 2):  # the first two warm up
                t.cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True)
                ms.append(t.last_ray_query_ms())
            out[f"{name} {w}x{h}"] = round(med(ms[2:]), 4)
            t.close()
    print(json.dumps(out))


def cast_on(lib, quick):
    env = dict(os.environ)
    env.pop("SRT_LIB", None)
    if lib:
        env["SRT_LIB"] = str(lib)
    r = subprocess.run([sys.executable, __file__, "--cast-child"] + (["--quick"] if quick else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"the cast on {lib or 'this library'} failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def id_pass_costs(quick, parent_lib):
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    here, parent = cast_on(None, quick), cast_on(parent_lib, quick) if parent_lib else {}
    out = []
    for name, scn, accel in scenes(S):
        for w, h in ([(960, 540)] if quick else [(960, 540), (1920, 1080)]):
            t = handle(R, S, Tracer, scn, accel, w, h)
            t.set_selection([0], width=2.0)
            t.clear_canvas()
            t.trace()
            first, cached = [], []
            for rep in range(REPS + 2):  # the first two warm up
                t.options["fov_scale"] = np.float32(1.0 + 1e-6 * (rep & 1))  # the key changes, the work does not
                t.trace()  # (the overlay's camera is the last dispatch's)
                first.append(resolve_ms(t))
                assert t.last_resolve_selected() == (True, True)
                cached.append(resolve_ms(t))
                assert t.last_resolve_selected() == (True, False)
            ids = t.read_id_pass()["shape"]
            key = f"{name} {w}x{h}"
            ms = med(first[2:]) - med(cached[2:])
            row = {"scene": name, "size": f"{w}x{h}", "pixels": w * h, "hits": int((ids != R.HIT_NONE).sum()), "id_pass_ms": round(ms, 4),
                   "resolve_first_ms": round(med(first[2:]), 4), "resolve_cached_ms": round(med(cached[2:]), 4), "cast_ms": here[key],
                   "id_pass_over_cast": round(ms / here[key], 3)}
            if parent:
                row["parent_cast_ms"], row["id_pass_over_parent_cast"] = parent[key], round(ms / parent[key], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            t.close()
    return out


def outline_costs(quick):
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S
    from simple_raytracer_amd.tracer import Tracer
    floor_cam = R.camera_matrix((20.0, 3.0, 20.0), 0.0, -1.5)
    cases = [("empty_mask", S.sphere_scene(), 0, S.default_camera(), [1000]), ("small_sphere", S.sphere_scene(), 0, S.default_camera(), [4]),
             ("mesh_silhouette", S.mesh_scene(), 1, S.default_camera(), [1]), ("full_screen_plane", S.sphere_scene(), 0, floor_cam, [0])]
    out = []
    for name, scn, accel, cam, sel in cases:
        for w, h in ([(960, 540)] if quick else [(960, 540), (1920, 1080)]):
            t = handle(R, S, Tracer, scn, accel, w, h)
            t.options["camera_to_world"] = cam
            t.clear_canvas()
            t.trace()
            row = {"case": name, "size": f"{w}x{h}"}
            for width in (2.0, 8.0):
                on, off = [], []
                for rep in range(REPS + 2):
                    t.set_selection(sel, width=width, fill=(96, 255, 160, 0))
                    resolve_ms(t)  # (makes the planes and uploads the tables)
                    on.append(resolve_ms(t))
                    assert t.last_resolve_selected() == (True, False)
                    t.set_selection()
                    off.append(resolve_ms(t))
                row[f"outline_ms_width{int(width)}"] = round(med(on[2:]) - med(off[2:]), 4)
                row[f"resolve_on_ms_width{int(width)}"], row["resolve_off_ms"] = round(med(on[2:]), 4), round(med(off[2:]), 4)
            t.set_selection(sel, width=2.0)
            resolve_ms(t)
            row["mask_share"] = round(float(np.isin(t.read_id_pass()["shape"], sel).mean()), 4)
            out.append(row)
            print(json.dumps(row), flush=True)
            t.close()
    return out


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
    if mode in ("on_still", "on_moving"):
        t.set_selection([4], width=2.0)
    cams = [R.camera_matrix((0.001 * (k % 64), 0.5, 5.0), 0.0, 0.0) for k in range(64)]
    out = np.zeros(w * h * 4, np.uint8)
    for rep in range(2):  # the first pass warms up
        t.clear_canvas()
        t.synchronize()
        t0 = time.perf_counter()
        for frame in range(FRAMES):
            t.options["time"] = np.uint32(1000 + frame)
            if mode == "on_moving":
                t.options["camera_to_world"] = cams[frame % 64]
            t.render_pipelined(frame + 1, out)
        t.pipeline_flush(out)
        dt = time.perf_counter() - t0
    print(json.dumps({"ms_per_frame": dt / FRAMES * 1e3}))
    t.close()


def loop(parent_lib):
    modes = [("off", None), ("on_still", None), ("on_moving", None)]
    if parent_lib:
        modes.insert(1, ("parent_library", parent_lib))
    runs = {m[0]: [] for m in modes}
    for rep in range(REPS):
        for name, lib in modes:  # in turn, so that drift of the box lands on all of them
            env = dict(os.environ)
            env.pop("SRT_LIB", None)
            if lib:
                env["SRT_LIB"] = str(lib)
            r = subprocess.run([sys.executable, __file__, "--loop-child", "off" if lib else name], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"{name}: the loop failed ({r.returncode}):\n{r.stdout}{r.stderr}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_frame"])
    res = {name: {"ms_per_frame_median": round(med(v), 4), "runs": [round(x, 4) for x in v], "spread": round(max(v) - min(v), 4)} for name, v in runs.items()}
    res["still_over_off"] = round(med(runs["on_still"]) / med(runs["off"]), 4)
    res["moving_over_off"] = round(med(runs["on_moving"]) / med(runs["off"]), 4)
    if parent_lib:
        res["off_over_parent"] = round(med(runs["off"]) / med(runs["parent_library"]), 4)
        res["off_minus_parent_ms"] = round(med(runs["off"]) - med(runs["parent_library"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="960x540 only")
    ap.add_argument("--loop-child", help=argparse.SUPPRESS)
    ap.add_argument("--cast-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child is not None:
        loop_child(a.loop_child)
        return
    if a.cast_child:
        cast_child(a.quick)
        return
    doc = {"id_pass": id_pass_costs(a.quick, a.parent_lib), "outline": outline_costs(a.quick)}
    doc["loop"] = loop(a.parent_lib)
    print(json.dumps({"loop": doc["loop"]}), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
