"""Device time of object motion for the temporal stage (srt_set_denoise_object_motion) against a baseline build of the
library (the parent commit's libsrt_hip.so), alternating the two builds in one session, and the quality while a shape is
dragged.

    python scripts/motion_probe.py --baseline-lib PATH/libsrt_hip.so [--rounds 5] [--reps 21] [--quality] [--out-dir profiles]

Each round starts one child process per build (a fresh process per library) that measures, with the library's HIP events:

  setup_camera_moved_ms   the temporal set-up after a camera move (the bilinear 2x2): srt_temporal_kernel<0, false, false> on both builds
  setup_object_moved_ms   this build, object motion on, one sphere moved since the history, camera still: srt_temporal_kernel<1, false, false>
  setup_both_moved_ms     the same with the camera moved too
  setup_nothing_moved_ms  object motion on, nothing moved, camera moved: the host launches srt_temporal_kernel<0, false, false>
  dispatch_ms             one 1-spp, 1-bounce dispatch with the denoiser on (trace + reduction + feature pass; the feature pass is
                          not timed alone); dispatch_ids_ms the same with object motion on (the feature pass stores the index)

Medians over --reps per child, then the median over the rounds. Scene: the sphere scene. --quality runs the protocol of
tests/test_gpu_denoise_motion.py::test_quality_dragged_shape and writes its three ratios per scene. Writes
r07_motion_<w>x<h>.json per size and r07_motion_quality.json to --out-dir.
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


def handle(lib, w, h, spp=2, bounces=10):
    shapes, tris, mats = S.sphere_scene()
    t = TR.Tracer(w, h, lib=lib)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, spp, bounces, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    return t, (shapes, tris, mats)


def resolve_ms(t, reps):
    out = []
    for _ in range(reps):
        t.resolve_denoised(1)
        out.append(t.last_kernel_ms()[1])
    return statistics.median(out[1:])


def dispatch_ms(t, reps):
    out = []
    t.set_kernel_timers(True)
    for i in range(reps):
        t.clear_canvas()
        t.options["time"] = 700 + i
        t.trace()
        t.synchronize()
        out.append(t.last_kernel_ms()[0])
    return statistics.median(out[1:])


def moved(shapes, dx):
    s = np.frombuffer(bytearray(shapes.tobytes()), shapes.dtype)
    s["sphere_position"][4, 0] += dx
    return s


def child(lib_path, w, h, reps):
    lib = TR._bind(C.CDLL(lib_path)) if lib_path else TR.load_library()
    has_motion = hasattr(lib, "srt_set_denoise_object_motion")
    cam1 = R.camera_matrix((0.013, 0.507, 4.989), 0.0, 0.0)
    r = {"has_motion": has_motion}

    def history(motion):
        t, scn = handle(lib, w, h)
        t.set_denoise(iterations=0)
        t.set_denoise_temporal()
        if motion:
            t.set_denoise_object_motion(True)
        t.trace()
        t.clear_canvas()
        return t, scn

    t, scn = history(False)
    t.options["camera_to_world"] = cam1
    t.trace()
    r["setup_camera_moved_ms"] = resolve_ms(t, reps)
    t.close()
    t, scn = handle(lib, w, h, 1, 1)
    t.set_denoise(iterations=0)
    t.set_denoise_temporal()
    r["dispatch_ms"] = dispatch_ms(t, reps)
    if has_motion:
        t.set_denoise_object_motion(True)
        r["dispatch_ids_ms"] = dispatch_ms(t, reps)
    t.close()
    if has_motion:
        for key, dx, cam in (("setup_object_moved_ms", 0.05, None), ("setup_both_moved_ms", 0.05, cam1), ("setup_nothing_moved_ms", 0.0, cam1)):
            t, (shapes, tris, mats) = history(True)
            t.update_scene(moved(shapes, dx) if dx else shapes, tris, mats)
            if cam is not None:
                t.options["camera_to_world"] = cam
            t.trace()
            assert t.read_denoise_history()["valid"] and t.read_denoise_motion()["any_moved"] == bool(dx)
            r[key] = resolve_ms(t, reps)
            t.close()
    print("RESULT " + json.dumps(r), flush=True)


def quality():
    import io
    from contextlib import redirect_stdout

    import test_gpu_denoise_motion as Q
    res = {}
    sky = S.synthetic_sky()
    for name in ("spheres", "meshes"):
        buf = io.StringIO()
        with redirect_stdout(buf):
            Q.test_quality_dragged_shape(TR, sky, name)
        line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("motion quality")][-1]
        res[name] = json.loads(line.split(": ", 1)[1])
        print(line, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--quality", action="store_true")
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
            res[side] = {k: statistics.median(r[k] for r in rs) for k in rs[0] if k != "has_motion"}
            res[side]["rounds_setup_camera_moved_ms"] = [r["setup_camera_moved_ms"] for r in rs]
        print(json.dumps(res), flush=True)
        if a.out_dir:
            p = Path(a.out_dir) / f"r07_motion_{w}x{h}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))
    if a.quality:
        q = quality()
        if a.out_dir:
            (Path(a.out_dir) / "r07_motion_quality.json").write_text(json.dumps(q, indent=1))


if __name__ == "__main__":
    main()
