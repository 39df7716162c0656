"""Cost of per-triangle materials (srt_set_triangle_materials) in the trace kernel's time, for the library that is loaded (SRT_LIB
selects another build, e.g. the parent commit's: run the probe once per build, alternating, and compare the lines).
960x540, 2 spp, ten bounces, the kernel's time from the library's event pair, medians and (min, max) over --reps dispatches
after one warm-up:
  a  the two-mesh and the 100k-triangle BVH scenes with a 1x1 texture bound and no table: both builds run the textured kernels
  b  the same with a per-face table (tm[k] = (k // 2) % n_materials, every fifth entry -1); only a build that has the setter
  c  plain scenes, nothing bound: the sphere scene and both BVH scenes (the untextured kernels)
One JSON line.
usage: triangle_materials_probe.py [--reps N]"""
import json, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import srt_pkg
srt_pkg.load()
from simple_raytracer_amd import records as R, scenes as S
from simple_raytracer_amd.tracer import Tracer, load_library

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
HAS_TABLE = hasattr(load_library(), "srt_set_triangle_materials")
SKY = S.synthetic_sky()
W, H, SPP = 960, 540, 2


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def trace_ms(scene, accel, textured, table):
    shapes, tris, mats = scene
    t = Tracer(W, H)
    t.set_skybox(SKY)
    t.set_acceleration(accel)
    t.set_kernel_timers(True)
    t.scene_data = R.scene_data(len(shapes))
    t.options = R.render_data(W, H, SPP, 10, camera_to_world=S.default_camera(), time=31337)
    t.update_scene(shapes, tris, mats)
    if textured:
        t.set_textures([np.full((1, 1, 4), 0.7, np.float32)])
        b = np.zeros(len(mats), R.MATERIAL_TEXTURE)
        for i in range(len(mats)):
            b[i] = R.material_texture(0, 0, 1.0, 1.0)
        t.set_material_textures(b)
    if table:
        k = np.arange(len(tris))
        t.set_triangle_materials(np.where(k % 5 == 4, -1, (k // 2) % len(mats)).astype(np.int32))
    out = []
    for i in range(REPS + 1):
        t.clear_canvas()
        t.trace()
        t.synchronize()
        out.append(t.last_kernel_ms()[0])
    assert bool(t.last_trace_textured()) == (textured or table)
    t.close()
    return stats(out[1:])


meshes = {"mesh2x1k": S.mesh_scene(2), "mesh100k": S.mesh_scene(1, 224, 224, smooth=False)}
res = {"has_table": HAS_TABLE, "reps": REPS, "a": {}, "b": {}, "c": {"spheres": trace_ms(S.sphere_scene(), 0, False, False)}}
for name, scene in meshes.items():
    res["a"][name] = trace_ms(scene, 1, True, False)
    if HAS_TABLE:
        res["b"][name] = trace_ms(scene, 1, True, True)
    res["c"][name] = trace_ms(scene, 1, False, False)
print(json.dumps(res))
