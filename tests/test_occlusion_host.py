"""Occlusion queries, the part that needs no device (include/srt_abi.h "occlusion queries"): the segment record's size and
layout, the mask's bit order, the header against records.py and the bindings, the argument errors the entry points report
before they touch a device, and the shared cases' own arithmetic."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import occlusion_cases as O
from simple_raytracer_amd import records as R, tracer as T

ROOT = Path(__file__).resolve().parent.parent
SRT_ERR_INVALID = 1
SYMBOLS = ("srt_occluded_rays", "srt_occluded_rays_device", "srt_occluded_segments", "srt_segment_rays", "srt_group_occluded_rays",
           "srt_group_occluded_segments", "srt_group_segment_rays", "srt_occlusion_sizes")


@pytest.fixture(scope="module")
def lib():
    from simple_raytracer_amd import build
    build.build_hip()
    return T.load_library()


def test_sizes_match_the_library(lib):
    out = (C.c_size_t * 2)()
    assert lib.srt_occlusion_sizes(out) == 0
    assert (out[0], out[1]) == (R.SEGMENT.itemsize, 8) == (32, 8)
    assert lib.srt_occlusion_sizes(None) == SRT_ERR_INVALID


def test_segment_layout_is_two_128_bit_words():
    assert [R.SEGMENT.fields[n][1] for n in ("from", "end_gap", "to", "reserved")] == [0, 12, 16, 28]
    s = R.segments((1, 2, 3), [(0, 0, -1), (0, 1, 0)], end_gap=[0.0, 2.5])
    assert s.dtype == R.SEGMENT and len(s) == 2 and np.array_equal(s["from"], [[1, 2, 3]] * 2) and s["end_gap"][1] == np.float32(2.5)
    words = s.view(np.uint32).reshape(2, 8)
    assert words[0, 0] == 0x3F800000 and words[0, 6] == 0xBF800000 and words[1, 3] == 0x40200000 and not words[:, 7].any()
    text = (ROOT / "include" / "srt_types.h").read_text()
    body = re.search(r"typedef struct srt_segment \{(.*?)\} srt_segment;", text, re.S).group(1)
    assert re.findall(r"^\s*float (\w+)", body, re.M) == ["from", "end_gap", "to", "reserved"]


def test_mask_bit_order():
    bits = np.zeros(130, bool)
    bits[[0, 5, 63, 64, 129]] = True
    words = O.words_of(bits)
    assert words.tolist() == [(1 << 0) | (1 << 5) | (1 << 63), 1 << 0, 1 << 1]
    assert np.array_equal(R.mask_bits(words, 130), bits) and len(R.mask_bits(words, 0)) == 0
    assert np.array_equal(R.mask_bits(np.asarray([0xFFFFFFFFFFFFFFFF], np.uint64), 3), [True] * 3)


def test_header_and_bindings_name_the_entry_points(lib):
    abi = (ROOT / "include" / "srt_abi.h").read_text()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\(", abi), sym
        assert sym in T.ABI_SYMBOLS and hasattr(lib, sym), sym
    for cls in (T.Tracer, T.TracerGroup):
        for name in ("occluded_rays", "occluded_segments", "segment_rays"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(T.Tracer.occluded_rays_device)
    assert abi.index("occlusion queries (new)") > abi.index("ray queries (new)")


def test_argument_errors_without_a_device(lib):
    """No handle: every entry point refuses before it looks at a device, whatever else it is given."""
    rays, segs, words = np.zeros(2, R.RAY), np.zeros(2, R.SEGMENT), np.zeros(2, np.uint64)
    p = T._ptr
    for flags in (0, R.RAYS_UNIT_DIRECTIONS, 2, 0x80000000):
        assert lib.srt_occluded_rays(None, p(rays), 2, flags, p(words), None) == SRT_ERR_INVALID
        assert lib.srt_occluded_rays_device(None, p(rays), 2, flags, p(words), None) == SRT_ERR_INVALID
        assert lib.srt_group_occluded_rays(None, p(rays), 2, flags, p(words), p(words)) == SRT_ERR_INVALID
    assert lib.srt_occluded_rays(None, None, 0, 0, None, None) == SRT_ERR_INVALID
    assert lib.srt_occluded_segments(None, p(segs), 2, p(words), None) == SRT_ERR_INVALID
    assert lib.srt_group_occluded_segments(None, p(segs), 2, p(words), None) == SRT_ERR_INVALID
    assert lib.srt_segment_rays(None, p(segs), 2, p(rays)) == SRT_ERR_INVALID
    assert lib.srt_group_segment_rays(None, p(segs), 2, p(rays)) == SRT_ERR_INVALID
    assert not words.any() and not rays.view(np.uint32).any()  # nothing was written


def test_the_shared_cases_are_what_they_say():
    """The directed ray sets aim where their names say (numpy alone), and the float64 restatement's bounds are the derived ones."""
    segs, answers = O.sphere_segments()
    assert len(segs) == len(answers) and {"visible", "occluded", "invalid"} == set(answers)
    direction, tmax, dir_bound, tmax_bound = O.segment_rays_f64(segs[:6])
    assert np.allclose(direction[0], (0, 0, -1)) and np.allclose(tmax[[0, 2, 3, 4, 5]], [10.0, 6.9, 7.1, 7.05, 6.95], atol=1e-6)
    # sphere 4's surface is 7 units from A along the segment: in front of 7.1 and 7.05, behind 6.9 and 6.95
    assert [bool(7.0 < x) for x in tmax[[2, 3, 4, 5]]] == [a == "occluded" for a in answers[2:6]]
    assert np.all(dir_bound <= 7 * O.U) and np.all(tmax_bound <= 12 * O.U * 10.0)
    r = O.random_segments()
    d = r["to"].astype(np.float64) - r["from"]
    assert len(r) == 257 and np.linalg.norm(d, axis=1).min() > 0.4 and (r["end_gap"] >= 0).all() and (r["end_gap"][::7] == 0).all()
    two = O.rays_two_models()
    assert len(two) == 64 and np.allclose(np.linalg.norm(two["direction"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (O.rays_one_lane_left(37)["direction"][37] == np.asarray((0.0, 0.8, 0.6), np.float32)).all()
    rays, bad = O.hostile_rays((0, 0, 5), (0, 0, -1), unit=False)
    assert len(rays) == 12 and bad == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]
