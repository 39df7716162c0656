"""GPU (MI355X): what a device group forwards (csrc/srt_group.hip) and the frame pipeline's own state (csrc/frame_pipeline.hip),
on virtual devices of one GPU. A group call is one of three families -- every member, the first member, the group's full-frame
resolver handle -- and a failure in any of them carries the member's code and text; the families share one group's state
(exposure, denoiser switch) without disturbing each other. A 16 x 7 frame on 3 members with rows_per_block = 2: the height is no
multiple of world * rows_per_block, so the padded rows exceed the owned ones and the last rank owns fewer rows than the first."""
import numpy as np
import pytest

import golden_io
from gpu_harness import T  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
W, H, N, RPB = 16, 7, 3, 2
SRT_ERR_INVALID, SRT_ERR_STATE = 1, 3
G = golden_io.load_cases()["spheres"]


def options(time=12345):
    rd = G["rd"].copy()
    rd["width"], rd["height"], rd["aspect_ratio"], rd["num_samples"] = W, H, np.float32(W) / np.float32(H), 2
    rd["time"] = np.uint32(time)
    return rd


def setup(t, sky):
    t.set_skybox(sky)
    t.options, t.scene_data = options(), G["sd"].copy()
    t.update_scene(G["shapes"], G["tris"], G["mats"])
    t.clear_canvas()
    return t


def group(T, sky):
    return setup(T.TracerGroup(W, H, N, rows_per_block=RPB), sky)


def frame(t, time):
    """one frame of its own: cleared, traced with `time`, resolved, read back"""
    t.clear_canvas()
    t.options["time"] = np.uint32(time)
    return t.render(1).copy()


def failure(call):
    with pytest.raises(Exception) as e:
        call()
    return e.value.code, str(e.value)


def test_a_failing_call_of_each_family_carries_the_members_code_and_text(T, sky):
    assert T.owned_rows(H, 0, N, RPB) == 3 and T.owned_rows(H, N - 1, N, RPB) == 2 and T.padded_rows(H, N, RPB) * N > H
    untouched = group(T, sky)
    want = frame(untouched, 777)
    untouched.close()
    grp = group(T, sky)
    # every member: srt_set_acceleration refuses an unknown mode; the first member: srt_set_exposure refuses key <= 0; the
    # resolver: srt_set_denoise refuses iterations > 8
    for call in (lambda t: t.set_acceleration(7), lambda t: t.set_exposure(key=-1.0), lambda t: t.set_denoise(iterations=9)):
        single = T.Tracer(W, H)
        code, text = failure(lambda: call(single))
        single.close()
        assert code == SRT_ERR_INVALID and text.startswith("srt_set_")
        assert failure(lambda: call(grp)) == (code, text)
        assert np.array_equal(frame(grp, 777), want)
    # the noise meter's calls demand the group's denoiser
    for call in (lambda: grp.meter_noise(), lambda: grp.set_noise_meter(), lambda: grp.read_noise()):
        code, text = failure(call)
        assert code == SRT_ERR_STATE and "the group's denoiser is off" in text, text
        assert np.array_equal(frame(grp, 777), want)
    # the range before the state: with the denoiser off a gamma in range is a state error, one out of range is not
    assert failure(lambda: grp.set_denoise_history_clamp(-1.0))[0] == SRT_ERR_INVALID
    assert failure(lambda: grp.set_denoise_history_clamp(1.0))[0] == SRT_ERR_STATE
    assert np.array_equal(frame(grp, 777), want)
    grp.close()


RAYS = 64


def rays():
    rng = np.random.RandomState(11)
    o = np.tile(np.float32([0.0, 0.5, 5.0]), (RAYS, 1))
    d = (rng.rand(RAYS, 3).astype(np.float32) - np.float32(0.5)) * np.float32([1.0, 0.6, 0.0]) + np.float32([0.0, 0.0, -1.0])
    return o, d


def test_interleaved_families_on_one_group(T, sky):
    """Frames, a cast and an AO pass between changes of the exposure (the first member's state, shared with the resolver by
    pointer) and of the denoiser switch: every result equals that of a fresh group that was given only what the step depends on."""
    exposure, denoise = dict(mode="manual", ev=1.25), dict(iterations=0)
    o, d = rays()
    grp = group(T, sky)
    got = {1: frame(grp, 101)}
    grp.set_exposure(**exposure)
    got[3] = frame(grp, 303)
    grp.set_denoise(**denoise)
    got[5] = frame(grp, 505)
    got[6] = grp.cast_rays(o, d)
    grp.render_ao(samples=1)
    got[7] = grp.read_ao()
    grp.set_denoise(False)
    got[9] = frame(grp, 909)
    grp.close()

    def fresh(*steps):
        f = group(T, sky)
        for s in steps:
            s(f)
        return f

    ex, dn = (lambda f: f.set_exposure(**exposure)), (lambda f: f.set_denoise(**denoise))
    for step, f, time in [(1, fresh(), 101), (3, fresh(ex), 303), (5, fresh(ex, dn), 505), (9, fresh(ex), 909)]:
        assert np.array_equal(frame(f, time), got[step]), step
        f.close()
    assert not np.array_equal(got[1], got[3])  # (the exposure reached the group's resolve)
    f = fresh()
    want = f.cast_rays(o, d)
    assert want.tobytes() == got[6].tobytes() and np.any(want["flags"] != 0)
    f.close()
    f = fresh()
    f.render_ao(samples=1)
    plane, samples = f.read_ao()
    assert samples == got[7][1] == 1 and plane.shape == (H, W) and np.array_equal(plane, got[7][0])
    f.close()


def test_pipeline_state_is_the_handles_own(T, sky):
    """Two pipelined frames and a flush, a partition change (the pipeline's buffers are made anew), pipelined frames again: every
    delivered frame is the blocking one of an equally partitioned handle. A partition change with a frame in flight is refused,
    and a handle goes away with a frame in flight as one that never pipelined does."""
    def blocking(partition, times):
        t = setup(T.Tracer(W, H), sky)
        t.set_partition(*partition)
        out = [frame(t, tm)[:t.owned_rows * W * 4] for tm in times]
        t.close()
        return out

    t = setup(T.Tracer(W, H), sky)
    t.set_partition(0, 1, 8)
    buf = np.zeros(W * H * 4, np.uint8)
    delivered = 0
    for partition, times in [((0, 1, 8), (11, 22)), ((0, 2, 2), (33, 44))]:
        t.set_partition(*partition)
        n = t.owned_rows * W * 4
        assert n == {1: 7, 2: 4}[partition[1]] * W * 4
        got = []
        for tm in times:  # (a frame of its own each, as blocking()'s)
            t.clear_canvas()
            t.options["time"] = np.uint32(tm)
            k = t.render_pipelined(1, buf)
            if k >= 0:
                assert k == delivered
                delivered += 1
                got.append(buf[:n].copy())
        assert t.pipeline_flush(buf) == delivered
        delivered += 1
        got.append(buf[:n].copy())
        assert t.pipeline_flush(buf) == -1
        for a, b in zip(got, blocking(partition, times), strict=True):
            assert np.array_equal(a, b), partition
    assert t.render_pipelined(1, buf) == -1  # in flight ...
    t.set_partition(0, 1, 8)                 # ... while the frame's size changes
    code, text = failure(lambda: t.render_pipelined(1, buf))
    assert (code, text) == (SRT_ERR_STATE, "srt_render_pipelined: partition changed with a frame in flight (srt_pipeline_flush first)")
    t.close()  # with that frame in flight: the release waits for the copy stream
    T.Tracer(W, H).close()  # never pipelined: nothing of the pipeline's to release
