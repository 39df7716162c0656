"""CPU: the denoiser's device-group interface (include/srt_abi.h srt_group_set_denoise ...) is exported, declared in the
header, bound by tracer.py, and checks its arguments before it touches a device: a NULL group is SRT_ERR_INVALID. The layout
helper of the gathered planes is pure host arithmetic."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GROUP_CALLS = ["srt_group_set_denoise", "srt_group_set_denoise_temporal", "srt_group_reset_denoise_history", "srt_group_resolve_denoised",
               "srt_group_read_denoised", "srt_group_read_denoise_inputs", "srt_group_read_denoise_history"]
SRT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def test_symbols_are_exported_declared_and_bound(T):
    lib = T.load_library()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include/srt_abi.h").read_text(), flags=re.S)
    for name in GROUP_CALLS + ["srt_unpermute_planes_device", "srt_partition_planes_floats"]:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in T.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for method in ("set_denoise", "set_denoise_temporal", "reset_denoise_history", "resolve_denoised", "read_denoised", "read_denoise_inputs",
                   "read_denoise_history"):
        assert getattr(T.TracerGroup, method) is getattr(T.Tracer, method)  # one implementation, keyword arguments included


def test_null_group_is_invalid(T):
    lib = T.load_library()
    d, tp = T.DenoiseParams(), T.TemporalParams()
    assert lib.srt_denoise_defaults(C.byref(d)) == 0 and lib.srt_temporal_defaults(C.byref(tp)) == 0
    buf = (C.c_float * 16)()
    counts = (C.c_uint32 * 2)()
    valid = C.c_int(0)
    assert lib.srt_group_set_denoise(None, C.byref(d)) == SRT_ERR_INVALID
    assert lib.srt_group_set_denoise(None, None) == SRT_ERR_INVALID
    assert lib.srt_group_set_denoise_temporal(None, C.byref(tp)) == SRT_ERR_INVALID
    assert lib.srt_group_reset_denoise_history(None) == SRT_ERR_INVALID
    assert lib.srt_group_resolve_denoised(None, 1) == SRT_ERR_INVALID
    assert lib.srt_group_read_denoised(None, buf) == SRT_ERR_INVALID
    assert lib.srt_group_read_denoise_inputs(None, buf, buf, buf, counts) == SRT_ERR_INVALID
    assert lib.srt_group_read_denoise_history(None, buf, buf, buf, None, C.byref(valid)) == SRT_ERR_INVALID
    assert lib.srt_unpermute_planes_device(None, None, None, None, None, 8, 8, 2, 4) == SRT_ERR_INVALID
    assert lib.srt_unpermute_planes_device(buf, buf, buf, buf, buf, 0, 8, 2, 4) == SRT_ERR_INVALID  # (checked before any launch)


@pytest.mark.parametrize("w,h,world,rpb", [(64, 48, 2, 8), (64, 40, 3, 5), (61, 29, 5, 2), (61, 29, 8, 1), (64, 48, 8, 8), (41, 37, 3, 3), (7, 1, 1, 8)])
def test_planes_layout(T, w, h, world, rpb):
    """Per rank: three float4 planes and one float plane of padded_rows * width pixels, the last padded to four floats --
    52 B per pixel of the padded rows, and every rank's slot starts on 16 bytes."""
    lib = T.load_library()
    plane = T.padded_rows(h, world, rpb) * w
    n = lib.srt_partition_planes_floats(w, h, world, rpb)
    assert n == 12 * plane + (plane + 3) // 4 * 4
    assert n % 4 == 0 and 0 <= n * 4 - 52 * plane < 16
    for bad in [(0, h, world, rpb), (w, -1, world, rpb), (w, h, 0, rpb), (w, h, world, 0)]:
        assert lib.srt_partition_planes_floats(*bad) == -1
