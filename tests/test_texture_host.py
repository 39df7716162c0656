"""CPU: the albedo-texture contract without a device. tests/texture_ref.py (the numpy restatement the GPU tests compare the
kernels with) on analytic cases; the plane frames of the host-only call srt_plane_frame_host against the float64 formula;
every SRT_ERR_INVALID case of the setters through srt_texture_check_host."""
import numpy as np
import pytest

import texture_ref as TR
from simple_raytracer_amd import build, records as R, tracer

F = np.float32


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return tracer.load_library()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def noise(w, h, seed=3):
    img = np.random.default_rng(seed).random((h, w, 4)).astype(F)
    return img


# ---- 1. the sampler --------------------------------------------------------------------------------------------------
def test_nearest_returns_stored_texels_bit_for_bit():
    img = noise(7, 5)
    xs, ys = np.meshgrid(np.arange(7), np.arange(5))
    u = ((xs.reshape(-1) + F(0.5)) / F(7)).astype(F)
    v = ((ys.reshape(-1) + F(0.5)) / F(5)).astype(F)
    got = TR.sample(img, TR.NEAREST, u, v)
    assert np.array_equal(bits(got), bits(img[ys.reshape(-1), xs.reshape(-1), :3]))
    one = np.full((4, 4, 4), F(0.3), F)
    rnd = np.random.default_rng(1).normal(0, 50, (1000, 2)).astype(F)
    assert np.array_equal(bits(TR.sample(one, TR.NEAREST, rnd[:, 0], rnd[:, 1], 3.0, -2.5)), bits(np.full((1000, 3), F(0.3))))


def test_linear_at_centres_and_midpoints():
    img = noise(8, 4)  # power-of-two sides: centres and midpoints are exact coordinates
    xs, ys = np.meshgrid(np.arange(8), np.arange(4))
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    u, v = ((xs + F(0.5)) / F(8)).astype(F), ((ys + F(0.5)) / F(4)).astype(F)
    assert np.array_equal(bits(TR.sample(img, TR.LINEAR, u, v)), bits(img[ys, xs, :3]))  # weights 1, 0, 0, 0
    um = ((xs + F(1.0)) / F(8)).astype(F)  # halfway to the next column (the last one wraps to column 0)
    got = TR.sample(img, TR.LINEAR, um, v)
    a, b = img[ys, xs, :3], img[ys, (xs + 1) % 8, :3]
    want = (F(0.5) * a + F(0.5) * b).astype(F)  # fma(0.5, b, 0.5 * a): both products exact, one rounding
    assert np.array_equal(bits(got), bits(want))


def test_repeat_and_negative_coordinates():
    img = noise(8, 4)
    rng = np.random.default_rng(5)
    u = (rng.integers(0, 64, 500) / F(64)).astype(F)  # exact in float, as u + 1 and u - 3 are
    v = (rng.integers(0, 64, 500) / F(64)).astype(F)
    for filt in (TR.LINEAR, TR.NEAREST):
        base = TR.sample(img, filt, u, v)
        assert np.array_equal(bits(TR.sample(img, filt, u + F(1), v)), bits(base))
        assert np.array_equal(bits(TR.sample(img, filt, u - F(3), v - F(2))), bits(base))
    # negative coordinates wrap to non-negative indices: -1/16 of an 8-wide image is column 7
    got = TR.sample(img, TR.NEAREST, np.array([-1 / 16], F), np.array([-1 / 8], F))
    assert np.array_equal(bits(got[0]), bits(img[3, 7, :3]))


def test_nan_and_inf_sample_texel_0_0():
    img = noise(6, 5)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, 0.25], F)
    for filt in (TR.LINEAR, TR.NEAREST):
        got = TR.sample(img, filt, bad[:4], np.full(4, 0.3, F))
        assert np.array_equal(bits(got), bits(np.tile(img[0, 0, :3], (4, 1))))
        got = TR.sample(img, filt, np.full(4, 0.3, F), bad[:4])
        assert np.array_equal(bits(got), bits(np.tile(img[0, 0, :3], (4, 1))))


def test_sphere_poles_and_seam():
    c, r = np.array([1, 2, 3], F), F(2)
    u, v = TR.sphere_uv(np.array([[1, 4, 3], [1, 0, 3], [3, 2, 3], [-1, 2, 3], [1, 2, 5]], F), c, r)
    assert v[0] == 1 and v[1] == 0 and v[2] == F(0.5)
    assert u[2] == F(0.5) and u[4] == F(0.75)  # +x: atan2pi(0, 1) = 0; +z: atan2pi(1, 0) = 0.5
    assert u[3] == F(1.0)  # -x, the seam: atan2pi(+0, -1) = 1; u = 1 repeats to u = 0
    img = noise(8, 4)
    assert np.array_equal(bits(TR.sample(img, TR.NEAREST, u[3:4], v[3:4])), bits(TR.sample(img, TR.NEAREST, np.zeros(1, F), v[3:4])))


def test_plane_uv_at_the_frame_vectors():
    n = np.array([0.0, 1.0, 0.0], F)
    T, B = TR.plane_frame(n)
    pos = np.array([2, -1, 5], F)
    u, v = TR.plane_uv(np.stack([pos + T, pos + B, pos]), pos, T, B)
    assert (u[0], v[0]) == (1, 0) and (u[1], v[1]) == (0, 1) and (u[2], v[2]) == (0, 0)


def test_model_uv():
    w0, w1 = np.array([0.25, 0.0, 1.0], F), np.array([0.5, 0.0, 0.0], F)
    w2 = (F(1) - w0 - w1).astype(F)
    u, v = TR.model_uv(w0, w1, w2)
    assert np.array_equal(u, w0) and np.array_equal(v, w1)
    uv = np.tile(np.array([[0.5, 2.0], [-1.0, 0.25], [3.0, -4.0]], F), (3, 1, 1))
    u, v = TR.model_uv(w0, w1, w2, uv)
    # (uv0 * w2 + uv1 * w0) + uv2 * w1 at (w0, w1, w2) = (1/4, 1/2, 1/4), (0, 0, 1), (1, 0, 0): every product and sum exact
    assert np.array_equal(u, np.array([0.125 - 0.25 + 1.5, 0.5, -1.0], F))
    assert np.array_equal(v, np.array([0.5 + 0.0625 - 2.0, 2.0, 0.25], F))


# ---- 2. plane frames from the library ------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, np.float64)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b).astype(F)).astype(np.float64)


def test_plane_frames_match_the_float64_formula(lib):
    rng = np.random.default_rng(11)
    for n in np.concatenate([rng.normal(0, 1, (300, 3)), rng.normal(0, 1, (100, 3)) * 10.0 ** rng.integers(-12, 12, (100, 1))]).astype(F):
        got = tracer.plane_frame_host(n)
        assert got is not None
        T, B = got
        n64 = n.astype(np.float64)
        a = np.zeros(3)
        a[int(np.argmin(np.abs(n64)))] = 1.0
        t = np.cross(a, n64)
        t /= np.linalg.norm(t)
        b = np.cross(n64, t)
        assert ulps(T, t).max() <= 1.0 and ulps(B, b).max() <= 1.0, n
        assert abs(np.dot(T.astype(np.float64), n64)) <= 1e-6 * np.linalg.norm(n64)
        want = TR.plane_frame(n)
        assert np.array_equal(bits(T), bits(want[0])) and np.array_equal(bits(B), bits(want[1]))  # the restatement the GPU tests use


def test_plane_frame_tie_rule(lib):
    cases = {(0, 1, 0): 0, (0, 0, 1): 0, (1, 0, 0): 1, (1, 1, 0): 2, (1, 1, 1): 0, (2, 1, 1): 1, (0, -3, 0): 0, (1, 0, 1): 1}
    for n, axis in cases.items():
        T, B = tracer.plane_frame_host(np.array(n, F))
        a = np.zeros(3)
        a[axis] = 1.0
        t = np.cross(a, np.array(n, np.float64))
        t /= np.linalg.norm(t)
        assert np.array_equal(T, t.astype(F)), (n, T, t)
        assert np.array_equal(B, np.cross(np.array(n, np.float64), t).astype(F))


def test_no_frame_for_zero_or_non_finite_normals(lib):
    for n in [(0, 0, 0), (-0.0, 0, 0), (np.nan, 1, 0), (0, np.inf, 0), (1, 2, -np.inf)]:
        assert tracer.plane_frame_host(np.array(n, F)) is None
        assert TR.plane_frame(np.array(n, F)) is None


# ---- 3. validation -----------------------------------------------------------------------------------------------------
def B(*rows):
    out = np.zeros(len(rows), R.MATERIAL_TEXTURE)
    for i, r in enumerate(rows):
        out[i] = R.material_texture(*r)
    return out


def test_validation(lib):
    ok, bad = 0, 1
    chk = tracer.texture_check_host
    assert chk(2, B((0, 0, 1, 1), (1, 1, 2, -3), (-1, 0, 1, 1))) == ok
    assert chk(0) == ok and chk(0, B((-1, 0, 1, 1))) == ok
    assert chk(2, B((2, 0, 1, 1))) == bad        # an index beyond the texture count
    assert chk(0, B((0, 0, 1, 1))) == bad
    assert chk(2, B((-2, 0, 1, 1))) == bad
    assert chk(2, B((0, 2, 1, 1))) == bad        # an unknown filter
    assert chk(2, B((0, -1, 1, 1))) == bad
    for s in (np.nan, np.inf, -np.inf):          # a scale that is not finite
        assert chk(2, B((0, 0, s, 1))) == bad and chk(2, B((0, 0, 1, s))) == bad
    assert chk(2, B((-1, 0, np.nan, 1))) == bad  # (checked whether bound or not)
    assert chk(1, None, uv_triangles=12, scene_triangles=12) == ok
    assert chk(1, None, uv_triangles=11, scene_triangles=12) == bad
    assert chk(1, None, uv_triangles=0, scene_triangles=12) == bad
    assert chk(1, None, uv_triangles=None, scene_triangles=12) == ok
    assert chk(tracer.MAX_TEXTURES) == ok and chk(tracer.MAX_TEXTURES + 1) == bad
    assert chk(1, images=[(True, 4, 4)]) == ok
    assert chk(1, images=[(False, 4, 4)]) == bad  # no texels
    assert chk(1, images=[(True, 0, 4)]) == bad and chk(1, images=[(True, 4, -1)]) == bad and chk(1, images=[(True, 16385, 1)]) == bad


def test_abi_symbols_and_record(lib):
    for sym in ("srt_set_textures", "srt_set_material_textures", "srt_set_triangle_uvs", "srt_group_set_textures",
                "srt_group_set_material_textures", "srt_group_set_triangle_uvs", "srt_last_trace_textured"):
        assert hasattr(lib, sym), sym
    assert R.MATERIAL_TEXTURE.itemsize == 16
