"""What an occlusion query costs (include/srt_abi.h "occlusion queries") beside the closest-hit cast it replaces. One JSON document:

  rows            the centre rays of a 1920x1080 and a 960x540 frame of the bench sphere scene, the two-mesh scene (array scan and
                  hierarchy) and the 99,904-triangle scene (hierarchy) -- scripts/ray_query_probe.py's rows -- in two sets:
                  `camera` (tmax = inf: most rays are occluded, the early exit applies) and `half` (tmax = half the distance of
                  the ray's closest hit: most rays are visible, nothing ends early). Per row, under the kernel timers
                  (srt_last_ray_query_ms) and taking turns REPS times: srt_occluded_rays_device of this library,
                  srt_cast_rays_device of this library, and -- with --parent-lib PATH, a build of the parent commit --
                  srt_cast_rays_device of that library: the baseline. Medians, the baseline's own spread (min, max), and the
                  ratio occlusion / baseline. The mask is compared with the cast's SRT_HIT_HIT on the way.
                  (profiles/r30_occlusion.json also holds `occlusion_keys_ms`, the walk's other stack form, measured by this
                  script when that form was still in the tree: profiles/r32_anyhit_key_stack_experiment.patch.)

    python scripts/occlusion_probe.py [--parent-lib PATH] [--out FILE] [--quick]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

from ray_query_probe import centre_rays  # noqa: E402

REPS = 5


def med(xs):
    return float(statistics.median(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libsrt_hip.so built from the parent commit: the baseline cast")
    ap.add_argument("--out", help="write the JSON document here as well")
    ap.add_argument("--quick", action="store_true", help="960x540 only")
    a = ap.parse_args()
    import torch
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records as R, scenes as S, tracer as T
    libs = {"this": T.load_library()}
    if a.parent_lib:
        libs["parent"] = T._bind(C.CDLL(str(a.parent_lib)))
        assert not hasattr(libs["parent"], "srt_occluded_rays"), "--parent-lib is not the parent commit's library"
    scenes = [("spheres", S.sphere_scene(), 0), ("mesh2_scan", S.mesh_scene(), 0), ("mesh2_bvh", S.mesh_scene(), 1),
              ("mesh100k_bvh", S.mesh_scene(1, 224, 224), 1)]
    sizes = [(960, 540)] if a.quick else [(1920, 1080), (960, 540)]
    cam = S.default_camera()
    dev = torch.device("cuda", 0)
    rows = []
    for name, (shapes, tris, mats), accel in scenes:
        for w, h in sizes:
            tr = {}
            for key, lib in libs.items():
                t = T.Tracer(w, h, lib=lib)
                t.set_acceleration(accel)
                t.scene_data = R.scene_data(len(shapes))
                t.update_scene(shapes, tris, mats)
                t.set_kernel_timers(True)
                tr[key] = t
            rays = centre_rays(R, cam, w, h)
            n = len(rays)
            hits = tr["this"].cast_rays(rays, unit=True)
            half = rays.copy()
            half["tmax"] = np.where(hits["flags"] & R.HIT_HIT, np.float32(0.5) * hits["t"], np.float32(np.inf)).astype(np.float32)
            hits_dev = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            occ_dev = torch.zeros(((n + 63) // 64,), dtype=torch.int64, device=dev)
            for set_name, rs in (("camera", rays), ("half", half)):
                rays_dev = torch.from_numpy(rs.view(np.int32).reshape(n, 8).copy()).to(dev)
                torch.cuda.synchronize()

                def occlusion(key):
                    tr[key].occluded_rays_device(rays_dev.data_ptr(), n, occ_dev.data_ptr(), unit=True)
                    return tr[key].last_ray_query_ms()

                def cast(key):
                    tr[key].cast_rays_device(rays_dev.data_ptr(), n, hits_dev.data_ptr(), unit=True)
                    return tr[key].last_ray_query_ms()

                modes = [("occlusion", occlusion, "this"), ("cast", cast, "this")]
                if "parent" in libs:
                    modes.append(("parent_cast", cast, "parent"))
                want = (tr["this"].cast_rays(rs, unit=True)["flags"] & R.HIT_HIT) != 0
                ms = {m[0]: [] for m in modes}
                for rep in range(REPS + 1):  # the first warms up; in turn, so that drift lands on all of them
                    for label, fn, key in modes:
                        ms[label].append(fn(key))
                        if rep == 0 and fn is occlusion:
                            assert np.array_equal(R.mask_bits(occ_dev.cpu().numpy().view(np.uint64), n), want), (name, set_name, label)
                row = {"scene": name, "size": f"{w}x{h}", "rays": n, "set": set_name, "occluded": int(want.sum())}
                for label in ms:
                    row[label + "_ms"] = round(med(ms[label][1:]), 4)
                base = "parent_cast" if "parent" in libs else "cast"
                row["baseline"] = base
                row["baseline_min_max_ms"] = [round(min(ms[base][1:]), 4), round(max(ms[base][1:]), 4)]
                row["occlusion_over_baseline"] = round(med(ms["occlusion"][1:]) / med(ms[base][1:]), 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
            for t in tr.values():
                t.close()
    doc = {"reps": REPS, "rows": rows}
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
