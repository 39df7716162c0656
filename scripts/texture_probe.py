"""Device time of the trace kernel with albedo textures against the untextured kernels and against a baseline build of the
library (the parent commit's libsrt_hip.so), the builds alternated in fresh processes.

    python scripts/texture_probe.py [--baseline-lib PATH/libsrt_hip.so] [--rounds 3] [--reps 9] [--out-dir profiles]

Per round one child process per build. A child measures, with the library's HIP events around srt_trace_kernel alone
(srt_last_trace_kernel_ms), the median over --reps dispatches of

  untextured   nothing bound: the untextured kernels (both builds)
  tex_1x1      every material on a 1x1 NEAREST texture of its own colour: the branch, the UV and the gathers, perfect locality
  tex_noise    every material on one 1024x1024 noise texture, LINEAR, 37 repeats per unit of UV: divergent gathers

at 960x540x2 spp and 1920x1080x64 spp on the sphere scene and on the two-mesh scene with the BVH (planar UVs). The parent
build measures `untextured` only. Writes r08_texture_cost.json to --out-dir: per case the median over the rounds of each
mode, the baseline's spread over its rounds, and the ratios to this build's untextured time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import srt_pkg  # noqa: E402

srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S, tracer as TR  # noqa: E402

SIZES = [(960, 540, 2), (1920, 1080, 64)]


def scene(name):
    if name == "spheres":
        shapes, tris, mats = S.sphere_scene()
        return shapes, tris, mats, None, 0
    shapes, tris, mats = S.mesh_scene(2)
    return shapes, tris, mats, S.planar_triangle_uvs(tris, 2.0), TR.ACCEL_BVH


def bind(n, texture_of, filt, scale=1.0):
    b = np.zeros(n, R.MATERIAL_TEXTURE)
    for i in range(n):
        b[i] = R.material_texture(texture_of(i), filt, scale, scale)
    return b


def child(reps):
    lib = TR.load_library()  # (SRT_LIB in the environment selects the baseline build)
    has_tex = hasattr(lib, "srt_set_textures")
    sky = S.synthetic_sky()
    noise = S.noise_texture()
    out = {}
    for name in ("spheres", "meshes_bvh"):
        shapes, tris, mats, uvs, accel = scene(name)
        for w, h, spp in SIZES:
            t = TR.Tracer(w, h, lib=lib)
            t.set_skybox(sky)
            t.set_acceleration(accel)
            t.options = R.render_data(w, h, spp, 10, camera_to_world=S.default_camera(), time=4242)
            t.scene_data = R.scene_data(len(shapes))
            t.update_scene(shapes, tris, mats)
            modes = ["untextured"] + (["tex_1x1", "tex_noise"] if has_tex else [])
            for mode in modes:
                if mode == "tex_1x1":
                    imgs = []
                    for m in mats:
                        img = np.ones((1, 1, 4), np.float32)
                        img[..., :3] = m["color"]
                        imgs.append(img)
                    t.set_textures(imgs)
                    t.set_material_textures(bind(len(mats), lambda i: i, TR.FILTER_NEAREST))
                    t.set_triangle_uvs(uvs)
                elif mode == "tex_noise":
                    t.set_textures([noise])
                    t.set_material_textures(bind(len(mats), lambda i: 0, TR.FILTER_LINEAR, 37.0))
                    t.set_triangle_uvs(uvs)
                ms = []
                for k in range(reps + 2):
                    t.clear_canvas()
                    t.options["time"] = 4242 + k
                    t.trace()
                    t.synchronize()
                    if k >= 2:  # two warm-up dispatches
                        ms.append(t.last_trace_kernel_ms())
                if has_tex:
                    assert t.last_trace_textured() == (mode != "untextured")
                out[f"{name}_{w}x{h}x{spp}/{mode}"] = statistics.median(ms)
            t.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    runs = {"baseline": [], "this": []}
    for _ in range(a.rounds):
        for which, lib in (("baseline", a.baseline_lib), ("this", "")):
            if which == "baseline" and not lib:
                continue
            env = dict(os.environ)
            env.pop("SRT_LIB", None)
            if lib:
                env["SRT_LIB"] = lib
            r = subprocess.run([sys.executable, __file__, "--child", "--reps", str(a.reps)], capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:  # a child that failed ends the probe: nothing more is started on the device
                sys.exit(f"{which} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[which].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    report = {"unit": "ms, srt_trace_kernel device time (HIP events), median of reps per process, median over rounds",
              "rounds": a.rounds, "reps": a.reps, "cases": {}}
    for case in sorted({k.split("/")[0] for k in runs["this"][0]}):
        c = {}
        for mode in ("untextured", "tex_1x1", "tex_noise"):
            c[mode] = statistics.median(r[f"{case}/{mode}"] for r in runs["this"])
        if runs["baseline"]:
            b = [r[f"{case}/untextured"] for r in runs["baseline"]]
            c["baseline_untextured"] = statistics.median(b)
            c["baseline_rounds"] = b
            c["baseline_spread"] = (max(b) - min(b)) / statistics.median(b)
        c["this_untextured_rounds"] = [r[f"{case}/untextured"] for r in runs["this"]]
        c["ratio_1x1"] = c["tex_1x1"] / c["untextured"]
        c["ratio_noise"] = c["tex_noise"] / c["untextured"]
        report["cases"][case] = c
        print(case, json.dumps(c))
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r08_texture_cost.json").write_text(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
