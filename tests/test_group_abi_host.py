"""CPU: the exports of the collection, device-group and frame-pipeline units (csrc/srt_collect.hip, csrc/srt_group.hip,
csrc/frame_pipeline.hip) are the ones include/srt_abi.h declares, and every one of them checks its arguments before it touches
a device: a NULL group is SRT_ERR_INVALID but for the few calls whose NULL answer is a value of their own, named below."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRT_ERR_INVALID = 1
NAMES = re.compile(r"srt_group_\w+|srt_comm_\w+|srt_gather|srt_\w*gathered\w*|srt_unpermute\w*_device|srt_partition_planes_floats|"
                   r"srt_render_pipelined|srt_pipeline_flush")
# group calls whose answer to a NULL group is not SRT_ERR_INVALID (test_null_group_quirks), and the constructor
QUIRKS = {"srt_group_create", "srt_group_destroy", "srt_group_last_error", "srt_group_size", "srt_group_tracer",
          "srt_group_last_setup_history_illumination", "srt_group_last_setup_history_clamp", "srt_group_last_filter_history_feedback"}


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, tracer
    build.build_hip()
    return tracer


def declared():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include/srt_abi.h").read_text(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(srt_\w+)\s*\(", header) if NAMES.fullmatch(m.group(1))}


def test_declared_and_exported_symbols_are_the_same_set(T):
    from simple_raytracer_amd import build
    T.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build_hip())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    exported = {n for n in exported if NAMES.fullmatch(n)}
    want = declared()
    assert len(want) >= 70 and QUIRKS <= want, sorted(want)  # (the header was read: the group calls alone are 65)
    assert want - exported == set(), "declared, not exported"
    assert exported - want == set(), "exported, not declared"


def zero(tp):
    return None if issubclass(tp, (C.c_void_p, C.c_char_p, C._Pointer)) else tp(0)


def test_every_group_call_refuses_a_null_group(T):
    lib = T.load_library()
    calls = sorted(n for n in declared() if n.startswith("srt_group_") and n not in QUIRKS)
    assert len(calls) >= 55
    for name in calls:
        fn = getattr(lib, name)
        assert fn.argtypes, name  # bound by tracer.py
        # the first argument is the group; behind a NULL one nothing else is looked at
        assert fn(None, *[zero(tp) for tp in fn.argtypes[1:]]) == SRT_ERR_INVALID, name
    # ... nor with every other argument in order
    out, buf = C.c_int(0), (C.c_float * 16)()
    assert lib.srt_group_last_filter_demodulated(None, C.byref(out)) == SRT_ERR_INVALID
    assert lib.srt_group_last_resolve_exposed(None, C.byref(out)) == SRT_ERR_INVALID
    assert lib.srt_group_read_canvas(None, buf) == SRT_ERR_INVALID
    assert lib.srt_group_get_counters(None, C.byref(T.Counters())) == SRT_ERR_INVALID


def test_null_group_quirks(T):
    lib = T.load_library()
    assert lib.srt_group_last_setup_history_illumination(None) == 0
    assert lib.srt_group_last_setup_history_clamp(None) == 0
    assert lib.srt_group_last_filter_history_feedback(None) == 0
    assert lib.srt_group_size(None) == 0
    assert lib.srt_group_tracer(None, 0) is None
    assert lib.srt_group_last_error(None) == b"srt_group: NULL"
    assert lib.srt_group_destroy(None) is None  # returns


def test_group_create_checks_its_counts_first(T):
    lib = T.load_library()
    for n_devices, rpb in [(0, 8), (1, 0), (0, 0), (-1, 8)]:
        g = C.c_void_p(1)
        assert lib.srt_group_create(16, 8, n_devices, None, rpb, C.byref(g)) == SRT_ERR_INVALID
        assert g.value is None
    assert lib.srt_group_create(16, 8, 0, None, 8, None) == SRT_ERR_INVALID


def test_handle_calls_refuse_null(T):
    lib = T.load_library()
    buf, n = (C.c_uint8 * 64)(), C.c_longlong(5)
    assert lib.srt_render_pipelined(None, None, 1, buf, C.byref(n)) == SRT_ERR_INVALID
    assert lib.srt_pipeline_flush(None, buf, C.byref(n)) == SRT_ERR_INVALID
    assert lib.srt_gather(None, 0) == SRT_ERR_INVALID
    assert lib.srt_comm_init(None, C.cast(buf, C.c_void_p), 0, 1) == SRT_ERR_INVALID
    assert lib.srt_comm_unique_id(None) == SRT_ERR_INVALID
    assert lib.srt_resolve_gathered(None, 1) == SRT_ERR_INVALID
    assert lib.srt_gathered_buffers(None, None, None) == SRT_ERR_INVALID
    assert lib.srt_read_gathered(None, None, None) == SRT_ERR_INVALID


def test_unpermute_hooks_check_before_any_launch(T):
    lib = T.load_library()
    p = C.c_void_p(C.addressof((C.c_float * 16)()))  # never read: every call below is refused
    i = C.c_int
    one, planes = lib.srt_unpermute_device, lib.srt_unpermute_planes_device
    assert one(None, p, i(8), i(8), i(2), i(4)) == SRT_ERR_INVALID and one(p, None, i(8), i(8), i(2), i(4)) == SRT_ERR_INVALID
    for k in range(5):
        ptrs = [None if j == k else p for j in range(5)]
        assert planes(*ptrs, 8, 8, 2, 4) == SRT_ERR_INVALID, k
    for w, h, world, rpb in [(0, 8, 2, 4), (-1, 8, 2, 4), (8, 0, 2, 4), (8, -3, 2, 4), (8, 8, 0, 4), (8, 8, 2, 0)]:
        assert one(p, p, i(w), i(h), i(world), i(rpb)) == SRT_ERR_INVALID, (w, h, world, rpb)
        assert planes(p, p, p, p, p, w, h, world, rpb) == SRT_ERR_INVALID, (w, h, world, rpb)


def test_planes_floats_refuses_empty_extents(T):
    lib = T.load_library()
    assert lib.srt_partition_planes_floats(0, 8, 2, 4) == -1
    assert lib.srt_partition_planes_floats(8, 8, 0, 4) == -1
    assert lib.srt_partition_planes_floats(8, 8, 2, 0) == -1
    assert lib.srt_partition_planes_floats(8, 8, 2, 4) == 12 * 32 + 32  # (padded rows: 4 per rank)
