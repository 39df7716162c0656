"""The ambient-occlusion reference (tests/ao_ref.py) on its own: the oracle's exports it is stated with, its seed arithmetic,
the distribution of its directions, and -- by the reference alone -- that every scene, frame and sample count of the GPU
comparisons (tests/test_gpu_ao.py) shows what those comparisons need. No GPU: the pixel centres' rays are
area_through_ref.host_rays, which agree with the device's to rounding; every statement here has slack for that."""
import numpy as np
import pytest

import ao_cases as A
import ao_ref as AR
import area_through_ref as XR

F = np.float32


# ---- the exports ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 7, 0x9E3779B9, 0xC0FFEE, 0xFFFFFFFF])
def test_random_direction_advances_the_seed_by_six_draws(seed, oracle):
    d, after = oracle.random_direction(seed)
    _, six = oracle.random_floats(seed, 6)
    assert after == six and after != seed
    again, _ = oracle.random_direction(seed)
    assert np.array_equal(d.view(np.uint32), again.view(np.uint32))
    nxt, _ = oracle.random_direction(after)  # the stream goes on: the next vector is another one
    assert not np.array_equal(d.view(np.uint32), nxt.view(np.uint32))


def test_random_direction_has_unit_length(oracle):
    """normalize3 = v * rsqrt(dot(v, v)): the dot's three roundings move the squared length by 3u, so the root by 1.5u, the
    reciprocal root is within an ulp = 2u and each product rounds once more: 4.5u on the length, u = 2^-24. 6u is
    asserted."""
    d = AR.random_directions(oracle, AR.item_seeds(3, 0, 4096)).astype(np.float64)
    err = np.abs(np.linalg.norm(d, axis=1) - 1.0)
    print(f"| |rd| - 1 |: worst {err.max() / A.U:.2f} x 2^-24")
    assert (err <= 6 * A.U).all()


def test_normalize3_is_the_oracles(oracle):
    v = np.array([[3.0, 0.0, 4.0], [0.0, 0.0, 2.0], [1.0, 1.0, 1.0], [-1e-3, 2e-3, 5e-4]], F)
    n = oracle.normalize3(v)
    assert n.shape == v.shape and n.dtype == F
    assert np.array_equal(n[1].view(np.uint32), np.array([0.0, 0.0, 1.0], F).view(np.uint32))
    assert (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0) <= 6 * A.U).all()
    assert np.array_equal(oracle.normalize3(v[2]).view(np.uint32), n[2].view(np.uint32))  # one vector or rows: the same call


# ---- the seed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0xFFFFFFFF, 0, 0x9E3779B9])
def test_the_seed_arithmetic_wraps_as_uint32(base):
    for first, n in ((0, 70), (24 * 16 * 64 - 5, 5), ((1 << 31) - 3, 3)):
        got = AR.item_seeds(base, first, n)
        assert got.dtype == np.uint32
        assert got.tolist() == [(base + item * 0x9E3779B9) % (1 << 32) for item in range(first, first + n)]
    assert AR.item_seeds(0xFFFFFFFF, 1, 1)[0] == 0x9E3779B8  # the first wrap


# ---- the law ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,normal", [(0, (0.0, 1.0, 0.0)), (0xFFFFFFFF, (0.6, 0.0, -0.8)), (0x9E3779B9, (-2.0, 1.0, 2.0))])
def test_the_reference_follows_the_cosine_law(base, normal, oracle):
    """Over n = 2^16 item seeds and one normal: c = dot(D, N) has mean 2/3 and variance 1/2 - 4/9 = 1/18, a tangential component
    has mean 0 and variance 1/4 (c^2 is uniform on [0, 1], so 1 - c^2 has mean 1/2, shared by two tangents). Each mean within
    5 sigma / sqrt(n)."""
    n = 1 << 16
    nrm = oracle.normalize3(np.asarray(normal, F))
    rd = AR.random_directions(oracle, AR.item_seeds(base, 0, n))
    total = nrm[None, :] + rd
    assert total.dtype == F
    d = oracle.normalize3(total).astype(np.float64)
    t1, t2 = A.tangents(nrm[None, :].astype(np.float64))
    c, a, b = d @ nrm.astype(np.float64), d @ t1[0], d @ t2[0]
    tol_c, tol_t = 5 * np.sqrt(1 / 18) / np.sqrt(n), 5 * np.sqrt(1 / 4) / np.sqrt(n)
    print(f"seed {base:#x}: mean cosine {c.mean():.6f} (2/3 +- {tol_c:.6f}), tangential means {a.mean():+.6f} {b.mean():+.6f} (+- {tol_t:.6f})")
    assert abs(c.mean() - 2.0 / 3.0) <= tol_c
    assert abs(a.mean()) <= tol_t and abs(b.mean()) <= tol_t
    assert (c > 0).all()


# ---- what the frames show -------------------------------------------------------------------------------------------------------
_surf = {}


def surfaces(oracle, name, w, h):
    if (name, w, h) not in _surf:
        _surf[(name, w, h)] = AR.surfaces(oracle, A.ref_scene(name), XR.host_rays(A.ref_rd(name, w, h)))
    return _surf[(name, w, h)]


@pytest.mark.parametrize("name", list(A.REF_VIEWS))
@pytest.mark.parametrize("w,h", A.REF_FRAMES)
def test_the_frames_show_what_the_comparisons_need(name, w, h, oracle):
    scn, (_, _, wanted, radius) = A.ref_scene(name), A.REF_VIEWS[name]
    surf = surfaces(oracle, name, w, h)
    has = surf["has"]
    assert 2 * has.sum() >= w * h + 8, (name, has.sum())
    if name in A.ENCLOSED:
        assert has.all()  # (a closed sphere around the camera: ao_cases.py)
    else:
        assert (~has).sum() >= 4, name
    for shape in wanted:  # every scene contributes pixels whose winner is what it was added for
        assert (surf["shape"] == shape).sum() >= 1, (name, shape)
    for s in A.REF_SAMPLES:
        words = AR.records(oracle, surf, s, seed=s, radius=radius)
        c = AR.counts(oracle, scn, words, s)
        assert np.array_equal(c == AR.NONE, ~has) and (c[has] <= s).all()
        if s > 1:
            assert (((c > 0) & (c < s))[has]).sum() >= 4, (name, s)  # neither open nor closed


def test_the_added_scenes_winners_are_what_they_were_added_for(oracle):
    w, h = 24, 16
    # glass, from inside: the geometric normal (P - centre) / r points along the ray, the reference's N against it
    surf = surfaces(oracle, "glass_inside", w, h)
    sh = A.ref_scene("glass_inside")[0]
    p = surf["org"].astype(np.float64) + surf["dir"].astype(np.float64) * surf["t"].astype(np.float64)[:, None]
    outward = (p - sh["sphere_position"][1].astype(np.float64)) / float(sh["sphere_radius"][1])
    assert (surf["shape"] == 1).all() and ((outward * surf["dir"]).sum(axis=1) > 0).all()
    assert np.allclose(surf["normal"], -outward, atol=1e-5)
    glass = A.ref_scene("glass_inside")  # no ray travels further than the diameter 2.4 before it meets the sphere again
    assert (AR.counts(oracle, glass, AR.records(oracle, surf, 4, radius=2.5), 4) == 4).all()
    # a shape without a material is a surface
    surf = surfaces(oracle, "spheres_bare", w, h)
    sh = A.ref_scene("spheres_bare")[0]
    assert sh["material"][4] == -1 and (sh["material"][:4] >= 0).all() and (surf["shape"] == 4).sum() >= 2
    same = surfaces(oracle, "spheres", w, h)
    assert all(np.array_equal(surf[k], same[k]) for k in ("has", "t", "shape", "normal"))
    # the rotated, non-uniformly scaled instances: the reference's normal is not the face's
    surf = surfaces(oracle, "boxes", w, h)
    on = np.isin(surf["shape"], (3, 4))
    assert on.sum() >= 8 and (surf["triangle"][on] >= 0).all() and (surf["triangle"][surf["shape"] == 0] == -1).all()
    # flat mesh
    surf = surfaces(oracle, "mesh_flat", w, h)
    assert (surf["shape"] == 1).sum() >= 64


def test_small_frames_hold_a_surface_and_none(oracle):
    assert surfaces(oracle, "spheres", 1, 1)["has"].all() and not surfaces(oracle, "mesh_smooth", 1, 1)["has"].any()
    for name in ("spheres", "mesh_smooth"):
        has = surfaces(oracle, name, 3, 2)["has"]
        assert has.any() and not has.all()


# ---- the records ------------------------------------------------------------------------------------------------------------------
def test_records_and_windows(oracle):
    w, h, s = 13, 7, 4
    surf = surfaces(oracle, "spheres", w, h)
    words = AR.records(oracle, surf, s, seed=0xFFFFFFFF, radius=2.5, bias=0.01)
    assert words.shape == (w * h * s, 8) and words.dtype == np.uint32 and not words[:, 7].any()
    per_ray = np.repeat(surf["has"], s)
    none = np.array([0, 0, 0, AR.NAN_BITS, 0, 0, 0, 0], np.uint32)
    assert (words[~per_ray] == none).all() and (words[per_ray, 3] == F(2.5).view(np.uint32)).all()
    o = words[:, :3].reshape(w * h, s, 3)
    assert (o == o[:, :1]).all()
    for first, n in ((1, 2), (w * h - 2, 2), (5, 7)):
        assert np.array_equal(AR.records(oracle, surf, s, seed=0xFFFFFFFF, radius=2.5, bias=0.01, first=first, n=n), words[first * s:(first + n) * s])
    # the origin moves with the bias alone, the direction with the seed alone
    other = AR.records(oracle, surf, s, seed=0, radius=2.5, bias=0.0)
    assert (other[per_ray, 4:7] != words[per_ray, 4:7]).any(axis=1).all() and (other[per_ray, :3] != words[per_ray, :3]).any(axis=1).all()
    lifted = words[per_ray, :3].view(F).astype(np.float64) - other[per_ray, :3].view(F)
    assert np.allclose(lifted, 0.01 * np.repeat(surf["normal"], s, axis=0)[per_ray], atol=1e-5)


def test_counts_on_scenes_with_known_answers(oracle):
    from simple_raytracer_amd import records as R
    rd = A.frame_rd(R.camera_matrix((0.0, 1.0, 5.0), 0.0, 0.0), 13, 7, 1)
    one = lambda *shapes: (R.concat(R.SHAPE, *[np.atleast_1d(x) for x in shapes]), np.zeros(0, R.TRIANGLE), np.atleast_1d(R.material(color=(0.8, 0.8, 0.8))))
    # a plane alone is open everywhere
    scn = one(R.plane(0, (0, 0, 0), (0, 1, 0)))
    surf = AR.surfaces(oracle, scn, XR.host_rays(rd))
    c = AR.counts(oracle, scn, AR.records(oracle, surf, 16), 16)
    assert surf["has"].any() and not surf["has"].all() and not c[surf["has"]].any() and (c[~surf["has"]] == AR.NONE).all()
    # inside a sphere everything is closed, unless the radius is short
    scn = one(R.sphere(0, (0, 1, 0), 10.0))
    surf = AR.surfaces(oracle, scn, XR.host_rays(rd))
    assert (AR.counts(oracle, scn, AR.records(oracle, surf, 16), 16) == 16).all()
    assert not AR.counts(oracle, scn, AR.records(oracle, surf, 16, radius=0.25, bias=0.01), 16).any()
    # no scene: no surface
    empty = (np.zeros(0, R.SHAPE), np.zeros(0, R.TRIANGLE), scn[2])
    surf = AR.surfaces(oracle, empty, XR.host_rays(rd))
    assert not surf["has"].any() and (AR.counts(oracle, empty, AR.records(oracle, surf, 2), 2) == AR.NONE).all()
    # a hostile camera: no ray is valid
    bad = A.hostile_rd(rd, np.nan)
    scn = one(R.sphere(0, (0, 1, 0), 10.0))
    assert not AR.surfaces(oracle, scn, XR.host_rays(bad))["has"].any()
