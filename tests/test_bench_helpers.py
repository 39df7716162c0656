"""CPU: the parts of bench.py that do not need a GPU -- the W_ops / W_bytes bookkeeping of
SURVEY.md 8(d) and the cpu_baseline leg (which is allowed to use oracle/)."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("srt_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_algorithmic_work_formula(bench):
    from simple_raytracer_amd import scenes as S
    shapes, _, _ = S.sphere_scene()  # 4 spheres + 3 planes
    c = {"rays": 1000, "paths": 200, "sky": 150, "tri_tests": 0, "tri_pass_u": 0}
    assert bench.w_ops(c, shapes) == 1000 * 4 * 17 + 1000 * 3 * 14 + 1000 * 3 + 800 * 250 + 150 * 40 + 200 * 30
    shapes, _, _ = S.mesh_scene(2)  # 1 plane + 2 models
    c = {"rays": 10, "paths": 4, "sky": 3, "tri_tests": 500, "tri_pass_u": 20}
    assert bench.w_ops(c, shapes) == 10 * 14 + 10 * 2 * 24 + 10 * 3 + 500 * 30 + 20 * 22 + 6 * 250 + 3 * 40 + 4 * 30
    assert bench.w_bytes({"paths": 100, "sky": 2}, 50, 1000, 10**9) == 24 * 100 + 32 * 50 + 1000 + 128


def test_cpu_baseline_leg(bench, sky):
    from oracle import oracle_py
    r = bench.cpu_baseline("spheres_256_16spp", sky, target_seconds=1.5)
    assert r["unit"] == "Mray/s" and r["value"] > 0 and r["cores"] >= 1 and r["mpath_per_s"] > 0
    if oracle_py.ref_available():
        assert r["kind"] == "reference" and r["reference_equals_port"] is True and "bit-identical" in r["sample"]
    else:
        assert r["kind"] == "port"


def _undump(d):
    """canvas.npy with its non-finite values put back from canvas_nonfinite.npy"""
    c = np.load(d / "canvas.npy")
    rows = np.load(d / "canvas_nonfinite.npy")
    assert rows.dtype == np.float64 and rows.ndim == 2 and rows.shape[1] == 2
    flat = c.reshape(-1)
    flat[rows[:, 0].astype(np.int64)] = np.array([np.nan, np.inf, -np.inf], np.float32)[rows[:, 1].astype(np.int64) - 1]
    return c


def test_dump_outputs(bench, tmp_path, monkeypatch):
    from conftest import bits_equal
    rng = np.random.default_rng(7)
    h, w = 6, 5
    canvas = rng.standard_normal((h + 2, w, 4)).astype(np.float32)  # (a one-rank canvas may carry padding rows)
    canvas[0, 0, :3] = np.nan  # a NaN-poisoned pixel, and overflowed channels
    canvas[2, 3, 1], canvas[4, 1, 2] = np.inf, -np.inf
    argb = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    bench.dump_outputs(tmp_path / "whole", canvas, argb)
    files = sorted(f.name for f in (tmp_path / "whole").glob("*.npy"))
    assert files == ["argb.npy", "canvas.npy", "canvas_nonfinite.npy"]
    for f in files:
        a = np.load(tmp_path / "whole" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    c, a = np.load(tmp_path / "whole" / "canvas.npy"), np.load(tmp_path / "whole" / "argb.npy")
    assert c.dtype == a.dtype == np.float32 and c.shape == (h, w, 3) and a.shape == (h, w, 4)
    assert len(np.load(tmp_path / "whole" / "canvas_nonfinite.npy")) == 5
    assert bits_equal(_undump(tmp_path / "whole"), canvas[:h, :, :3]) and np.array_equal(a, argb.astype(np.float32))
    # over the budget: a fixed, seeded sample of the pixels, the same on every run
    monkeypatch.setattr(bench, "DUMP_BUDGET", 10 * (28 + 8))
    for d in ("s1", "s2"):
        bench.dump_outputs(tmp_path / d, canvas, argb)
    idx = np.load(tmp_path / "s1" / "pixel_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) <= 10 and np.all(np.diff(idx) > 0)
    for f in ("pixel_index.npy", "canvas.npy", "canvas_nonfinite.npy", "argb.npy"):
        got = np.load(tmp_path / "s1" / f)
        assert np.isfinite(got).all() and np.array_equal(got, np.load(tmp_path / "s2" / f)), f
    k = idx.astype(np.int64)
    assert bits_equal(_undump(tmp_path / "s1"), canvas[:h, :, :3].reshape(-1, 3)[k])
    assert np.array_equal(np.load(tmp_path / "s1" / "argb.npy"), argb.reshape(-1, 4)[k].astype(np.float32))
    # a finite canvas: no rows
    bench.dump_outputs(tmp_path / "finite", np.nan_to_num(canvas, nan=0.0, posinf=0.0, neginf=0.0), argb)
    assert np.load(tmp_path / "finite" / "canvas_nonfinite.npy").shape == (0, 2)
