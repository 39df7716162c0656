"""CPU: the moved-camera cases of tests/temporal_cases.py under the numpy restatement alone (tests/temporal_ref.py), on
frames of the oracle's feature pass -- few pixels are flagged `borderline`, and every case reaches the branch of the set-up
kernel it is there for. tests/test_gpu_denoise_temporal_cases.py runs the same cases on the device."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref as TR
from gpu_harness import scene

_frames = {}


def frames(oracle, scn, name, w, h):
    """(history frame, its record, current frame, its record, the history frame's shape indices) of a case; a frame is made
    once per camera"""
    arrays = TC.nan_scene() if scn == "nan" else scene(scn)
    out, ids = [], []
    for k, cam in enumerate(TC.CASES[name]):
        rdata = TC.render_record(w, h, cam, time=2000 + k)
        key = (scn, w, h, rdata.tobytes())
        if key not in _frames:
            _frames[key] = TC.features_frame(oracle, rdata, *arrays)
        out += [_frames[key][0], rdata]
        ids.append(_frames[key][1])
    return (*out, ids[0])


@pytest.mark.parametrize("w,h", TC.SIZES)
@pytest.mark.parametrize("name", TC.NAMES)
def test_cases_flag_few_pixels_and_reach_their_branch(oracle, name, w, h):
    hist_f, hist_rd, cur, cur_rd, _ = frames(oracle, "mixed", name, w, h)
    hist = TC.first_history(hist_f, hist_rd)
    rep = TR.reproject(cur, hist, cur_rd)
    flagged = int(rep["borderline"].sum())
    covered = cur["cov"] > 0
    counts = np.bincount(rep["taps"][covered], minlength=5)
    print(f"{name} {w}x{h}: {flagged} pixels flagged ({flagged / (w * h) * 100:.3f} %), pixels by tap count {counts.tolist()}")
    assert flagged <= (0.002 * w * h if (w, h) == (128, 72) else 1)
    assert covered.sum() > 0.4 * w * h
    assert not TR.same_camera(cur_rd, hist_rd)  # every case goes to TP_PROJECT (or, singular, to TP_NONE), none to the identity tap
    win = TC.window(cur, hist_rd, cur_rd)
    has = rep["h"] > 0
    if name == "hist_singular":
        assert win is None and TR.invert_rotation(hist_rd) is None and not has.any()
        return
    if name == "about_face":
        assert not win["in_front"][covered].any() and not has.any()
        return
    assert np.all(counts[1:] > 0), counts  # a 2x2 that loses none, one, two and three of its taps
    if TC.sees_past_the_border(name, w, h):
        assert (has & ((win["x0"] == -1) | (win["x0"] == w - 1) | (win["y0"] == -1) | (win["y0"] == h - 1))).any()
    if name in TC.MOSTLY_OUTSIDE:
        assert (covered & ~win["inside"]).sum() > 0.25 * covered.sum()
    if name in ("hist_scaled", "hist_mirror_shear"):  # a transposed read of R_h^-1 is another matrix
        m = TR._rotation(hist_rd)
        assert np.abs(TR.inv3(m) - m.T).max() > 0.1


def test_pure_changes_of_fov_or_aspect_alone_project():
    """the render record's two floats are part of the camera: a change of either alone is no identity tap"""
    a = TC.render_record(37, 29, (TC.GENERIC, 1.0, None))
    assert TR.same_camera(a, TC.render_record(37, 29, (TC.GENERIC, 1.0, None)))
    assert not TR.same_camera(a, TC.render_record(37, 29, (TC.GENERIC, 0.8, None)))
    assert not TR.same_camera(a, TC.render_record(37, 29, (TC.GENERIC, 1.0, 1.5)))


@pytest.mark.parametrize("w,h", TC.SIZES)
def test_a_non_finite_history_colour_costs_single_taps(oracle, w, h):
    """`dolly` over the sphere scene whose large sphere had no finite colour in the history. Under the thresholds (-1, 10)
    nothing but the colour tells the sphere's taps from the others, so along its outline a 2x2 loses one to three taps to
    the colour and keeps the rest. (Under the defaults depth and normal separate the outline first in these frames of
    first hits; on the device the NaN also reaches the sphere's surroundings by way of bounces, and the GPU test asserts the
    same under the defaults.)"""
    hist_f, hist_rd, cur, cur_rd, hist_ids = frames(oracle, "nan", "dolly", w, h)
    hist = TC.first_history(hist_f, hist_rd)
    shapes = TC.nan_scene()[0]
    on = np.isin(hist_ids, np.flatnonzero(shapes["material"] == TC.NAN_MATERIAL))
    assert on.any() and not on.all()
    hist["colour"] = hist["colour"].copy()
    hist["colour"][on, 0] = np.nan
    taps, lost = TC.taps_lost_to_colour(cur, hist, cur_rd, normal_threshold=-1.0, depth_threshold=10.0)
    partly = (lost >= 1) & (lost <= 3) & (taps >= 1)
    print(f"{w}x{h}: {int(partly.sum())} pixels lose one to three taps to the colour and keep one")
    assert partly.any() and (lost == 4).any()
