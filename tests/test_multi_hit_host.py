"""Multi-hit ray queries, the part that needs no device (include/srt_abi.h "multi-hit ray queries"): the library's sizes and its
host-only argument check, the header's constants against records.py, and the reference's own tie and order rules
(tests/multi_hit_ref.py sort_candidates, the authority of tests/test_gpu_multi_hit.py) on hand-made lists."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import multi_hit_ref as M
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
SRT_ERR_INVALID = 1
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from simple_raytracer_amd import build
    build.build_hip()
    return T.load_library()


def test_sizes_match_the_library(lib):
    out = (C.c_size_t * 3)()
    assert lib.srt_multi_hit_sizes(out) == 0
    assert tuple(out) == (R.RAY.itemsize, R.RAY_HIT.itemsize, R.MULTI_HIT_MAX) == (32, 32, 8)
    assert lib.srt_multi_hit_sizes(None) == SRT_ERR_INVALID


def test_check_host_over_k_and_flags(lib):
    known = R.RAYS_UNIT_DIRECTIONS | R.RAYS_COUNT_ALL
    assert known == 3
    for k, ok in ((0, False), (1, True), (8, True), (9, False)):
        for flags in (0, R.RAYS_UNIT_DIRECTIONS, R.RAYS_COUNT_ALL, known):
            assert lib.srt_multi_hit_check_host(k, flags) == (0 if ok else SRT_ERR_INVALID), (k, flags)
    for k in (1, 8):
        for flags in (4, 8, 0x80000000, known | 4, 0xFFFFFFFF):
            assert lib.srt_multi_hit_check_host(k, flags) == SRT_ERR_INVALID, (k, flags)
    assert lib.srt_multi_hit_check_host(0xFFFFFFFF, 0) == SRT_ERR_INVALID


def test_header_constants_and_symbols():
    text = (ROOT / "include" / "srt_types.h").read_text()

    def const(name):
        m = re.search(rf"#define {name} (0x[0-9a-fA-F]+|\d+)u", text)
        assert m, name
        return int(m.group(1), 0)

    assert const("SRT_RAYS_COUNT_ALL") == R.RAYS_COUNT_ALL and const("SRT_MULTI_HIT_MAX") == R.MULTI_HIT_MAX
    assert const("SRT_RAYS_COUNT_ALL") & const("SRT_RAYS_UNIT_DIRECTIONS") == 0
    abi = (ROOT / "include" / "srt_abi.h").read_text()
    for sym in ("srt_cast_rays_multi", "srt_cast_rays_multi_device", "srt_pick_through", "srt_group_cast_rays_multi", "srt_group_pick_through",
                "srt_multi_hit_check_host", "srt_multi_hit_sizes"):
        assert re.search(rf"\b{sym}\(", abi), sym
        assert sym in T.ABI_SYMBOLS and hasattr(T.load_library(), sym), sym


def test_argument_errors_without_a_handle(lib):
    rays, hits, counts = np.zeros(2, R.RAY), np.zeros((2, 2), R.RAY_HIT), np.zeros(2, np.uint32)
    rd = R.as_records(R.render_data(8, 4), R.RENDER_DATA)
    xy = np.zeros((2, 2), F)
    p = T._ptr
    assert lib.srt_cast_rays_multi(None, p(rays), 2, 2, 0, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_cast_rays_multi_device(None, p(rays), 2, 2, 0, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_pick_through(None, p(rd), p(xy), 2, 2, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_group_cast_rays_multi(None, p(rays), 2, 2, 0, p(hits), p(counts)) == SRT_ERR_INVALID
    assert lib.srt_group_pick_through(None, p(rd), p(xy), 2, 2, p(hits), p(counts)) == SRT_ERR_INVALID
    assert not hits.view(np.uint32).any() and not counts.any()


# ---- the reference's own rules, on hand-made lists -----------------------------------------------------------------------------
def test_duplicate_spheres_tie_goes_to_array_order():
    got = M.sort_candidates([(F(2.0), 5, None), (F(2.0), 3, None), (F(1.0), 9, None)], np.inf)
    assert [(c[1]) for c in got] == [9, 3, 5]


def test_equal_t_inside_a_model_goes_to_the_lower_triangle():
    got = M.sort_candidates([(F(2.0), 1, 7), (F(2.0), 1, 2), (F(2.0), 0, 11), (F(2.0), 1, 5)], np.inf)
    assert [(c[1], c[2]) for c in got] == [(0, 11), (1, 2), (1, 5), (1, 7)]


def test_negative_zero_ties_with_positive_zero():
    # -0 == +0 as floats: the shape index decides, not the sign bit
    got = M.sort_candidates([(F(0.0), 4, None), (F(-0.0), 6, None), (F(-0.0), 2, None)], np.inf)
    assert [c[1] for c in got] == [2, 4, 6]
    assert np.signbit(got[0][0]) and not np.signbit(got[1][0])  # t as computed is kept


def test_nan_t_is_no_candidate():
    got = M.sort_candidates([(F(np.nan), 0, None), (F(1.0), 1, None), (F(np.nan), 2, 3)], np.inf)
    assert [c[1] for c in got] == [1]
    assert M.sort_candidates([(F(1.0), 0, None)], np.nan) == []


def test_tmax_is_strict():
    cands = [(F(1.0), 0, None), (F(2.0), 1, None), (F(3.0), 2, None), (F(4.0), 3, None)]
    assert [c[1] for c in M.sort_candidates(cands, F(3.0))] == [0, 1]
    assert [c[1] for c in M.sort_candidates(cands, np.nextafter(F(3.0), F(np.inf)))] == [0, 1, 2]
    assert [c[1] for c in M.sort_candidates(cands, np.inf)] == [0, 1, 2, 3]
    assert M.sort_candidates(cands, F(0.0)) == [] and M.sort_candidates(cands, F(-1.0)) == []
