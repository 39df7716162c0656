"""Device time of the temporal set-up with the history clamp off and on (srt_set_denoise_history_clamp), for a moved camera and
for a moved shape.

  setup_off_ms   srt_resolve_denoised with K = 0, temporal on, a history, the clamp off: the set-up kernel of a library without
                 the switch (library HIP events around the filter)
  setup_on_ms    the same frame with the clamp on (gamma 1): srt_temporal_bounds_kernel and the clamping set-up kernel, the two
                 launches together (the library's events surround the filter, not each launch)
  added_ms       setup_on_ms - setup_off_ms: what the switch costs a frame

camera: the camera moved since the history (srt_temporal_kernel<0, false, false> / <0, false, true>); shape: the camera still, object motion on
and one sphere moved (srt_temporal_kernel<1, false, false> / <1, false, true>). Switch off and on alternate in one process on one handle and
one canvas; medians of --reps rounds (default 7) after one round that is thrown away. Scene: scenes.sphere_scene, 2 spp. Writes
profiles/r20_history_clamp_<w>x<h>.json to --out-dir. With a library that lacks the switch (SRT_LIB: a parent checkout's build)
only the off figures are reported: the parent's set-up time by the same probe.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import build as B, records as R, scenes as S, tracer as TR  # noqa: E402


def cam_at(k):
    return R.camera_matrix((0.013 * k, 0.5 + 0.007 * k, 5.0 - 0.011 * k), 0.0, 0.0)


def probe(w, h, reps, moved):
    shapes, tris, mats = S.sphere_scene()
    t = TR.Tracer(w, h)
    t.set_skybox(S.synthetic_sky())
    t.options = R.render_data(w, h, 2, 10, camera_to_world=S.default_camera(), time=1234)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.set_denoise(iterations=0)
    t.set_denoise_temporal()
    if moved == "shape":
        t.set_denoise_object_motion(True)
    t.trace()
    t.clear_canvas()  # the history, at the default camera
    if moved == "shape":
        now = shapes.copy()
        now["sphere_position"][4] += (0.05, 0.02, 0.03)
        t.update_scene(now, tris, mats)
    else:
        t.options["camera_to_world"] = cam_at(1)
    t.options["time"] = 1235
    t.trace()
    has_switch = hasattr(t.lib, "srt_set_denoise_history_clamp")
    ms = {False: [], True: []}
    for rep in range(reps + 1):
        for on in ((False, True) if has_switch else (False,)):
            if has_switch:
                t.set_denoise_history_clamp(1.0 if on else 0.0)
            t.resolve_denoised(1)
            v = t.last_kernel_ms()[1]
            if has_switch:
                assert t.last_setup_history_clamp() == on
            if rep:
                ms[on].append(v)
    r = {"setup_off_ms": statistics.median(ms[False]), "setup_off_ms_all": ms[False]}
    if has_switch:
        r.update({"setup_on_ms": statistics.median(ms[True]), "setup_on_ms_all": ms[True]})
        r["added_ms"] = r["setup_on_ms"] - r["setup_off_ms"]
    t.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--tag", default="", help="appended to the file name (a parent checkout's run: _parent)")
    a = ap.parse_args()
    B.build_hip()
    for s in a.sizes.split(","):
        if not s:
            continue
        w, h = (int(v) for v in s.split("x"))
        res = {"width": w, "height": h, "spp": 2, "reps": a.reps, "scene": "sphere_scene", "gamma": 1.0,
               "camera": probe(w, h, a.reps, "camera"), "shape": probe(w, h, a.reps, "shape")}
        print(json.dumps(res), flush=True)
        if a.out_dir:
            p = Path(a.out_dir) / f"r20_history_clamp_{w}x{h}{a.tag}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
