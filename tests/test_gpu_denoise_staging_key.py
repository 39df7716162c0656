"""GPU: a setter between a filter and the clear. The commit at a clear trusts the set the filter staged only when the staging key
(csrc/denoise_plan.h) of the settings as they are at the clear equals the key the filter staged under, and makes the set itself
when not -- so the committed history never depends on when a setter was called. Two shapes of test, both bit for bit:
  a change    handle `a` filters, changes a setting, clears; handle `b` changes it first and only traces; their histories are
              equal -- and, where the setting is one the staging set depends on, differ from that of a handle that kept it
  a no-op     handle `a` filters, calls setters that leave every setting as it was (A -> B -> A, the same values again),
              clears; its history equals that of a handle that never called them
The transitions of one switch (illumination, clamp, feedback on / off, K and the sigmas under the feedback) are in
test_gpu_denoise_history_illumination.py, ..._history_clamp.py and ..._history_feedback.py."""
import pytest

from conftest import bits_equal
from gpu_harness import T, cam_at  # noqa: F401 (T: the fixture)
from test_gpu_denoise_history_clamp import TP, handle, same_history

pytestmark = pytest.mark.gpu
W, H = 64, 48


def aim(t, k):
    """frame k's scene, camera and seed"""
    t.update_scene(*t.scene)
    t.options["camera_to_world"] = cam_at(k, "move")
    t.options["time"] = 70 + k


def committed(handles, frames):
    """`frames` frames rendered and committed on every handle alike"""
    for k in range(frames):
        for t in handles:
            aim(t, k)
            t.render(1)
            t.clear_canvas()


CHANGES = {
    # name: (handle's switches, the change, whether the staging set depends on what changes)
    "history_limit": (dict(gamma=0.0), lambda t: t.set_denoise_temporal(**dict(TP, history_limit=1)), True),
    "clamp_sigma_normal": (dict(gamma=1.0, K=2), lambda t: t.set_denoise(iterations=2, sigma_normal=8.0), True),
    # the bounds launch takes no luminance weight and without the feedback no pass is staged: the key stays equal, rightly
    "clamp_sigma_luminance": (dict(gamma=1.0, K=2), lambda t: t.set_denoise(iterations=2, sigma_luminance=0.5), False),
}


@pytest.mark.parametrize("name", sorted(CHANGES))
def test_a_change_between_the_filter_and_the_clear(T, sky, name):
    kw, change, depends = CHANGES[name]
    a, b, kept = (handle(T, sky, "spheres", W, H, **kw) for _ in range(3))
    committed((a, b, kept), 2)  # two frames of history: counts above 1 for history_limit = 1 to bind, a history for the clamp
    for t in (a, b, kept):
        aim(t, 2)
    a.render(1)
    change(a)
    change(b)
    b.trace()
    kept.render(1)
    for t in (a, b, kept):
        t.clear_canvas()
    ha, hb, hk = (t.read_denoise_history() for t in (a, b, kept))
    same_history(ha, hb)
    if depends:
        assert not (bits_equal(ha["colour"], hk["colour"]) and bits_equal(ha["count"], hk["count"])), "the change changes nothing: the test shows nothing"
    else:
        same_history(ha, hk)
    for t in (a, b, kept):
        t.close()


def again(**dn):
    return lambda t: (t.set_denoise(**dn), t.set_denoise_temporal(**TP))


NOOPS = {
    # name: (handle's switches, history feedback, the calls that leave every setting as it was, group members)
    "illumination": (dict(illum=True, K=1), False, lambda t: (t.set_denoise_history_illumination(False), t.set_denoise_history_illumination(True)), 0),
    "clamp_gamma": (dict(gamma=1.0, K=1), False, lambda t: (t.set_denoise_history_clamp(2.0), t.set_denoise_history_clamp(1.0)), 0),
    "feedback": (dict(gamma=0.0, K=2), True, lambda t: (t.set_denoise_history_feedback(False), t.set_denoise_history_feedback(True)), 0),
    "same_values": (dict(gamma=1.0, K=2), True, again(iterations=2), 0),
    "same_values_group": (dict(gamma=1.0, K=2, illum=True), True, lambda t: (again(iterations=2)(t), t.set_denoise_history_clamp(0.0), t.set_denoise_history_clamp(1.0)), 2),
}


@pytest.mark.parametrize("name", sorted(NOOPS))
def test_a_setter_that_changes_nothing(T, sky, name):
    kw, feedback, calls, group = NOOPS[name]
    a, never = (handle(T, sky, "spheres", W, H, group=group, **kw) for _ in range(2))
    for t in (a, never):
        t.set_denoise_history_feedback(feedback)
    for k in range(3):
        for t in (a, never):
            aim(t, k)
            t.render(1)
        calls(a)
        for t in (a, never):
            t.clear_canvas()
        same_history(a.read_denoise_history(), never.read_denoise_history())
        if feedback:  # the clear took the set the filter staged: it ran no pass 1 of its own over the filter's image
            assert bits_equal(a.read_denoised(), never.read_denoised()), k
    assert a.last_setup_history_clamp() == never.last_setup_history_clamp() == bool(kw.get("gamma", 1.0))
    a.close()
    never.close()
