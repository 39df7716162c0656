"""Ray queries, the part that needs no device (include/srt_abi.h "ray queries"): the records' sizes and layout, the header's
constants against records.py, and the argument errors the entry points report before they touch a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
SRT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from simple_raytracer_amd import build
    build.build_hip()
    return T.load_library()


def test_record_sizes_match_the_library(lib):
    out = (C.c_size_t * 2)()
    assert lib.srt_ray_query_sizes(out) == 0
    assert (out[0], out[1]) == (R.RAY.itemsize, R.RAY_HIT.itemsize) == (32, 32)
    assert lib.srt_ray_query_sizes(None) == SRT_ERR_INVALID


def test_record_layouts_are_two_128_bit_words():
    assert [R.RAY.fields[n][1] for n in ("origin", "tmax", "direction", "reserved")] == [0, 12, 16, 28]
    assert [R.RAY_HIT.fields[n][1] for n in ("t", "shape", "triangle", "material", "normal", "flags")] == [0, 4, 8, 12, 16, 28]
    r = R.rays((1, 2, 3), [(0, 0, -1), (0, 1, 0)], tmax=[np.inf, 2.5])
    assert r.dtype == R.RAY and len(r) == 2 and np.array_equal(r["origin"], [[1, 2, 3]] * 2) and r["tmax"][1] == np.float32(2.5)
    words = r.view(np.uint32).reshape(2, 8)
    assert words[0, 3] == 0x7F800000 and words[1, 5] == 0x3F800000 and not words[:, 7].any()


def test_header_constants_match_records():
    text = (ROOT / "include" / "srt_types.h").read_text()

    def const(name):
        m = re.search(rf"#define {name} (0x[0-9a-fA-F]+|\d+)u", text)
        assert m, name
        return int(m.group(1), 0)

    assert const("SRT_RAYS_UNIT_DIRECTIONS") == R.RAYS_UNIT_DIRECTIONS
    assert (const("SRT_HIT_HIT"), const("SRT_HIT_FRONT"), const("SRT_HIT_INVALID_RAY")) == (R.HIT_HIT, R.HIT_FRONT, R.HIT_INVALID_RAY)
    assert const("SRT_HIT_NONE") == R.HIT_NONE == 0xFFFFFFFF
    abi = (ROOT / "include" / "srt_abi.h").read_text()
    for sym in ("srt_cast_rays", "srt_cast_rays_device", "srt_pick", "srt_group_cast_rays", "srt_group_pick", "srt_last_ray_query_ms",
                "srt_ray_query_sizes"):
        assert re.search(rf"\b{sym}\(", abi), sym
        assert sym in T.ABI_SYMBOLS and hasattr(T.load_library(), sym), sym


def test_argument_errors_without_a_device(lib):
    """No handle: every entry point refuses before it looks at a device, whatever else it is given."""
    rays, hits = np.zeros(2, R.RAY), np.zeros(2, R.RAY_HIT)
    rd = R.as_records(R.render_data(8, 4), R.RENDER_DATA)
    xy = np.zeros((2, 2), np.float32)
    p = T._ptr
    for flags in (0, R.RAYS_UNIT_DIRECTIONS, 2, 0x80000000):
        assert lib.srt_cast_rays(None, p(rays), 2, flags, p(hits)) == SRT_ERR_INVALID
        assert lib.srt_cast_rays_device(None, p(rays), 2, flags, p(hits)) == SRT_ERR_INVALID
        assert lib.srt_group_cast_rays(None, p(rays), 2, flags, p(hits)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays(None, None, 2, 0, None) == SRT_ERR_INVALID
    assert lib.srt_cast_rays(None, None, 0, 0, None) == SRT_ERR_INVALID
    assert lib.srt_pick(None, p(rd), p(xy), 2, p(hits)) == SRT_ERR_INVALID
    assert lib.srt_pick(None, None, None, 2, None) == SRT_ERR_INVALID
    assert lib.srt_group_pick(None, p(rd), p(xy), 2, p(hits)) == SRT_ERR_INVALID
    ms = C.c_float(-1.0)
    assert lib.srt_last_ray_query_ms(None, C.byref(ms)) == SRT_ERR_INVALID
    assert not hits.view(np.uint32).any()  # nothing was written


@pytest.mark.parametrize("name", ["spheres", "boxes", "mesh_smooth", "mesh_flat"])
def test_cameras_give_hits_and_misses(name, oracle):
    """The cameras of tests/ray_query_cases.py make the device comparison one of hits and of misses, and the second camera is
    not the scene's default (the CPU oracle alone)."""
    import ray_query_cases as Q
    hits = np.concatenate([np.isfinite(Q.primary(oracle, name, k)[2]["t"]) for k in (0, 1)])
    assert hits.sum() >= 8 and (~hits).sum() >= 8, (name, int(hits.sum()), int((~hits).sum()))
    assert not np.allclose(Q.CAMERAS[name][0], Q.CAMERAS[name][1])
    dirs = Q.primary(oracle, name, 1)[2]["dir"].astype(np.float64)
    assert np.all(np.abs((dirs * dirs).sum(axis=1) - 1.0) < 1e-6)
