"""GPU: the host side of the device BVH upkeep (csrc/accel_device.hip) where one handle lives through several uploads: its two
pinned read-backs (the deform cost sums, the sorted order) shrink and regrow, a read-back nobody asks for is overtaken by the
next upload, the two timed spans are of the last upload only, a group's first member hands its whole policy to the others, and
a handle is destroyed with and without the events and pinned buffers ever made. Every mode on: SRT_ACCEL_BVH,
SRT_REFIT_DEVICE, SRT_DEFORM_REFIT, SRT_BUILD_DEVICE with min_triangles 0. Frames are 16x16, 1 sample, 3 bounces."""
import ctypes as C

import numpy as np
import pytest

import bvh_build_cases as B
import bvh_deform_cases as D
import test_gpu_bvh_deform as G
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
DEVICE, REFIT = 1, 1
MORTON, MEDIAN = 0, 1
W = H = 16
SMALL, LARGE = "n13", "p300"  # 13 triangles of the blob; the first 300 of n6k


def handle(T, sky, order=MORTON, accel=1):
    t = T.Tracer(W, H)
    t.set_skybox(sky)
    t.set_acceleration(accel)
    t.set_acceleration_refit(DEVICE)
    t.set_acceleration_deform(REFIT)
    t.set_acceleration_build(DEVICE, 0)
    t.set_acceleration_build_order(order)
    t.options = R.render_data(W, H, 1, 3, camera_to_world=S.default_camera(), time=4711)
    return t


def upload(t, name):
    tris = B.mesh(name)
    G.update(t, G.scene(D.shape_over(tris)), tris)


def state(t):
    """what the getters say of the last upload, the blocks as bytes"""
    return {"build": t.acceleration_build_info(), "deform": t.acceleration_deform_info(), "refit": t.acceleration_refit_info(),
            "acc": {k: v for k, v in t.acceleration_info().items() if k != "build_us"}, "blocks": t.read_bvh_blocks().tobytes()}


def canvas(t):
    t.clear_canvas()
    t.trace()
    return t.read_canvas()


@pytest.mark.parametrize("order", [MORTON, MEDIAN])
def test_read_backs_shrink_and_regrow(order, T, sky):
    fresh = {}
    for name in (SMALL, LARGE):
        t = handle(T, sky, order)
        upload(t, name)
        fresh[name] = state(t)
        t.close()
    assert fresh[SMALL]["build"]["records"] == 13 and fresh[LARGE]["build"]["records"] == 300
    assert fresh[LARGE]["refit"]["models"] == 1 and fresh[LARGE]["deform"]["cost_launches"] >= 1
    assert fresh[SMALL]["blocks"] != fresh[LARGE]["blocks"]
    t = handle(T, sky, order)
    for name in (SMALL, LARGE, SMALL):
        upload(t, name)
        assert state(t) == fresh[name], name
    t.close()


def test_read_back_nobody_consumes(T, sky):
    t = handle(T, sky)
    upload(t, LARGE)
    upload(t, SMALL)  # (no getter in between, none before the trace)
    got = canvas(t)
    t.close()
    scan = handle(T, sky, accel=0)
    upload(scan, SMALL)
    want = canvas(scan)
    scan.close()
    assert bits_equal(got, want) and want.any()


def test_timed_spans_are_the_last_uploads(T, sky):
    t = handle(T, sky)
    t.set_kernel_timers(True)
    upload(t, LARGE)
    assert t.acceleration_build_info()["models"] == 1 and t.acceleration_refit_info()["models"] == 1
    assert t.last_build_kernel_ms() > 0.0 and t.last_refit_kernel_ms() > 0.0
    G.update(t, G.scene(), B.mesh(SMALL))  # the plane alone
    assert t.last_build_kernel_ms() == 0.0 and t.last_refit_kernel_ms() == 0.0
    t.set_kernel_timers(False)
    upload(t, LARGE)
    assert t.acceleration_build_info()["models"] == 1 and t.acceleration_refit_info()["models"] == 1
    assert t.last_build_kernel_ms() == 0.0 and t.last_refit_kernel_ms() == 0.0
    t.close()


def test_policy_reaches_every_member(T, sky):
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=2)
    g.set_skybox(sky)
    lib, first = g.lib, g.member(0)
    assert lib.srt_set_acceleration(first, 1) == 0 and lib.srt_set_acceleration_refit(first, DEVICE) == 0
    assert lib.srt_set_acceleration_deform(first, REFIT, 4.0) == 0 and lib.srt_set_acceleration_build(first, DEVICE, 7) == 0
    assert lib.srt_set_acceleration_build_order(first, MEDIAN) == 0
    tris = B.mesh(LARGE)
    G.update(g, G.scene(D.shape_over(tris)), tris)

    def member_state(i):
        refit, n = (C.c_uint64 * 4)(), C.c_size_t(0)
        assert lib.srt_acceleration_refit_info(g.member(i), refit) == 0
        assert lib.srt_read_bvh_blocks(g.member(i), None, 0, C.byref(n)) == 0
        blocks = np.zeros((n.value, 32), np.uint32)
        assert lib.srt_read_bvh_blocks(g.member(i), blocks.ctypes.data_as(C.c_void_p), len(blocks), C.byref(n)) == 0
        return g.member_build_info(i), g.member_deform_info(i)["cost_launches"], list(refit), blocks.tobytes()

    states = [member_state(i) for i in range(2)]
    g.close()
    assert states[0][0]["models"] == 1 and states[0][0]["launches"] > 0 and states[0][1] >= 1 and states[0][2][0] == 1 and len(states[0][3]) > 0
    assert states[1] == states[0]
    single = handle(T, sky, MEDIAN)  # ... and the order was the first member's: the blocks are a single handle's under MEDIAN
    upload(single, LARGE)
    assert single.read_bvh_blocks().tobytes() == states[0][3]
    single.close()


def test_life_cycle(T, sky):
    for _ in range(2):
        t = handle(T, sky)
        t.set_kernel_timers(True)
        upload(t, LARGE)
        t.close()  # both read-backs pending, both spans recorded
    t = T.Tracer(W, H)  # never uploaded: no event, no pinned buffer
    t.close()
    t = handle(T, sky)  # a HIP error of the destroyed handles would be this one's first
    upload(t, SMALL)
    assert t.acceleration_build_info()["models"] == 1
    t.close()
