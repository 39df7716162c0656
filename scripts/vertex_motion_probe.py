"""Device time of per-triangle motion for the temporal stage (srt_set_denoise_vertex_motion) against a baseline build of the
library (the parent commit's libsrt_hip.so), alternating the two builds in one session.

    python scripts/vertex_motion_probe.py --baseline-lib PATH/libsrt_hip.so [--rounds 5] [--reps 21] [--out-dir profiles]

Each round starts one child process per build (a fresh process per library) that measures, with the library's HIP events:

  setup_camera_moved_ms   the temporal set-up after a camera move, every switch off: srt_temporal_kernel<0, false, false> on both builds
  setup_model_moved_ms    this build, mesh scene (two 968-triangle instances, BVH), object motion on, one instance translated,
                          camera still: srt_temporal_kernel<1, false, false>
  setup_deformed_ms       the same scene, per-triangle motion on, the mesh waved since the history, camera still:
                          srt_temporal_kernel<2, false, false> (both instances' pixels project)
  setup_deformed_cam_ms   the same with the camera moved too (every pixel projects)
  dispatch_ms             one 1-spp, 1-bounce dispatch of the mesh scene with the denoiser on (trace + reduction + feature pass);
                          dispatch_ids_ms with object motion on, dispatch_tris_ms with per-triangle motion on (the triangle-index store)
  big_dispatch_ms         the same dispatch over the 99,904-triangle mesh with per-triangle motion on and the scene unchanged;
  big_dispatch_table_ms   ... after an srt_update_scene with waved vertices: the dispatch also writes the world-vertex table
                          (the difference is the table launch)

Medians over --reps per child, then the median over the rounds. Writes r17_vertex_motion_<w>x<h>.json to --out-dir.
"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S, tracer as TR  # noqa: E402

import motion_ref as M  # noqa: E402
import vertex_motion_ref as V  # noqa: E402


def handle(lib, scn, w, h, spp=2, bounces=10, accel=1):
    shapes, tris, mats = scn
    t = TR.Tracer(w, h, lib=lib)
    t.set_skybox(S.synthetic_sky())
    t.set_acceleration(accel)
    t.options = R.render_data(w, h, spp, bounces, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t


def resolve_ms(t, reps):
    out = []
    for _ in range(reps):
        t.resolve_denoised(1)
        out.append(t.last_kernel_ms()[1])
    return statistics.median(out[1:])


def dispatch_ms(t, reps, before=None):
    out = []
    t.set_kernel_timers(True)
    for i in range(reps):
        t.clear_canvas()
        if before:
            before(i)
        t.options["time"] = 700 + i
        t.trace()
        t.synchronize()
        out.append(t.last_kernel_ms()[0])
    return statistics.median(out[1:])


def child(lib_path, w, h, reps):
    lib = TR._bind(C.CDLL(lib_path)) if lib_path else TR.load_library()
    has = hasattr(lib, "srt_set_denoise_vertex_motion")
    cam1 = R.camera_matrix((0.013, 0.507, 4.989), 0.0, 0.0)
    r = {"has_vertex_motion": has}
    meshes = S.mesh_scene()
    shapes, tris, mats = meshes

    def history(motion, vertex):
        t = handle(lib, meshes, w, h)
        t.set_denoise(iterations=0)
        t.set_denoise_temporal()
        if motion:
            t.set_denoise_object_motion(True)
        if vertex:
            t.set_denoise_vertex_motion(True)
        t.trace()
        t.clear_canvas()
        return t

    t = history(False, False)
    t.options["camera_to_world"] = cam1
    t.trace()
    r["setup_camera_moved_ms"] = resolve_ms(t, reps)
    t.close()
    t = handle(lib, meshes, w, h, 1, 1)
    t.set_denoise(iterations=0)
    t.set_denoise_temporal()
    r["dispatch_ms"] = dispatch_ms(t, reps)
    t.set_denoise_object_motion(True)
    r["dispatch_ids_ms"] = dispatch_ms(t, reps)
    if has:
        t.set_denoise_vertex_motion(True)
        r["dispatch_tris_ms"] = dispatch_ms(t, reps)
    t.close()
    if has:
        t = history(True, False)
        t.update_scene(M.move_shapes(shapes, tris, [(1, "translate", (0.05, 0.02, 0.0))], 1), tris, mats)
        t.trace()
        assert t.read_denoise_history()["valid"] and t.read_denoise_motion()["any_moved"]
        r["setup_model_moved_ms"] = resolve_ms(t, reps)
        t.close()
        for key, cam in (("setup_deformed_ms", None), ("setup_deformed_cam_ms", cam1)):
            t = history(True, True)
            t.update_scene(shapes, V.wave(tris, 12, 968, 1), mats)
            if cam is not None:
                t.options["camera_to_world"] = cam
            t.trace()
            assert t.read_denoise_history()["valid"] and (t.read_denoise_motion()["state"] == V.DEFORMED).sum() == 2
            r[key] = resolve_ms(t, reps)
            t.close()
        big = S.mesh_scene(1, 224, 224)
        n = len(big[1]) - 12
        t = handle(lib, big, w, h, 1, 1)
        t.set_acceleration_refit(TR.REFIT_DEVICE)
        t.set_acceleration_deform(TR.DEFORM_REFIT)
        t.update_scene(*big)
        t.set_denoise(iterations=0)
        t.set_denoise_temporal()
        t.set_denoise_object_motion(True)
        t.set_denoise_vertex_motion(True)
        r["big_dispatch_ms"] = dispatch_ms(t, reps)
        waves = [V.wave(big[1], 12, n, k, amplitude=0.002) for k in (1, 2)]
        r["big_dispatch_table_ms"] = dispatch_ms(t, reps, before=lambda i: t.update_scene(big[0], waves[i & 1], big[2]))
        r["big_triangles"] = n
        t.close()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0] if a.child[0] != "-" else None, int(a.child[1]), int(a.child[2]), a.reps)
        return
    for s in [v for v in a.sizes.split(",") if v]:
        w, h = (int(v) for v in s.split("x"))
        sides = {"this": "-"}
        if a.baseline_lib:
            sides = {"baseline": a.baseline_lib, "this": "-"}
        runs = {k: [] for k in sides}
        for _ in range(a.rounds):
            for side, lib in sides.items():  # alternating: baseline, this, baseline, this, ...
                out = subprocess.run([sys.executable, __file__, "--reps", str(a.reps), "--child", lib, str(w), str(h)], capture_output=True, text=True,
                                     timeout=300, check=True).stdout
                runs[side].append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        res = {"width": w, "height": h, "rounds": a.rounds, "reps": a.reps}
        for side, rs in runs.items():
            res[side] = {k: statistics.median(r[k] for r in rs) for k in rs[0] if k != "has_vertex_motion"}
            res[side]["rounds_setup_camera_moved_ms"] = [r["setup_camera_moved_ms"] for r in rs]
        print(json.dumps(res), flush=True)
        if a.out_dir:
            p = Path(a.out_dir) / f"r17_vertex_motion_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
