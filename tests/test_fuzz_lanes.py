"""CPU: the lanes of tests/fuzz_scenes.py test what they claim -- without a GPU, with the oracle alone. Every lane at its
default count: the restatement of the library's kernel choice gives the lane's intended class for every scene; the near
misses cover every edit; the moved generator draws the scenes it drew before the move; the restatement's material flags are
those the library's thresholds give; and the hostile scenes are not NaN or sky all over (a canvas that is proves nothing)."""
import hashlib

import numpy as np
import pytest

import fuzz_scenes as FS
from simple_raytracer_amd import records as R, tracer as T

# sha256 over the first 20 scenes (shapes, triangles, materials, camera, render and scene records) per seed of
# test_random_scenes_match_oracle, computed from random_scene as it stood in tests/test_gpu_fuzz.py before the move
PARENT_HASHES = {20240: "669c88bfff8fec0a7a72c1ced0b448901bda3cf2fe46db8927086e23b48a1ff4",
                 20241: "3d7fb5808b0c7b2eab276db21e4552b478e160410b492825588383a68e69ee84"}
CASES = [(name, hostile) for name in FS.LANES for hostile in (False, True)]
_scenes = {}


def lane_scenes(name, hostile):
    """every scene of the case at its default count, as run_lane draws them"""
    if (name, hostile) not in _scenes:
        rng = np.random.RandomState(FS.lane_seed(name, hostile))
        _scenes[name, hostile] = [FS.LANES[name](rng, hostile, it) for it in range(FS.lane_iterations(name))]
    return _scenes[name, hostile]


@pytest.mark.parametrize("seed", sorted(PARENT_HASHES))
def test_moved_generator_draws_the_same_scenes(seed):
    hostile = bool(seed - 20240)
    rng = np.random.RandomState(seed)
    h = hashlib.sha256()
    for _ in range(20):
        shapes, tris, mats, cam = FS.random_scene(rng, hostile)
        rd, sd = FS.random_options(rng, shapes, cam, 24, 16)
        for a in (shapes, tris, mats, cam, rd, sd):
            h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == PARENT_HASHES[seed]


def test_the_old_importers_still_find_the_generator():
    import test_gpu_fuzz
    assert test_gpu_fuzz.random_scene is FS.random_scene


@pytest.mark.parametrize("name,hostile", CASES)
def test_restatement_gives_the_intended_class(name, hostile):
    """100 % of every lane: class lanes their class, near misses their fallback, general and textured lanes class 0"""
    scenes = lane_scenes(name, hostile)
    for it, (shapes, tris, mats, cam, rd, sd, expected, extra) in enumerate(scenes):
        assert FS.expected_class(shapes, mats, rd, textured=expected[1]) == expected[0], (name, hostile, it, extra.get("what"))
        assert int(sd["num_shapes"]) == len(shapes)
        if name in FS.CLASS_LANES:
            assert tuple(expected) == (FS.CLASS_LANES[name], False)
        elif name != "near_miss":
            assert expected[0] == FS.GENERAL
        if name.startswith(("tex_", "texvar_")):
            assert expected[1] == (not rd["show_normals"])
            assert FS.expected_class(shapes, mats, rd) == (FS.CLASS_LANES[f"class{it % 4 + 1}"] if name.endswith("_class") else FS.GENERAL)
        if name.startswith("texvar_"):
            tex = extra["textures"]
            assert all(np.isfinite(im).all() and (im >= 0).all() and not np.signbit(im).any() for im in tex["images"])
            assert np.isfinite(tex["bindings"]["scale_u"]).all() and np.isfinite(tex["bindings"]["scale_v"]).all()
    if name in ("scan_pad", "bvh_pad"):
        assert all(FS.scene_lds_bytes(len(s[0]), len(s[2])) == 0 for s in scenes)
    if name.startswith("texvar_"):  # every branch of the image generator: both filters, 1x1 and larger, a refused NaN scale when hostile
        assert {int(f) for s in scenes for f in s[7]["textures"]["bindings"]["filter"]} == {0, 1}
        shapes_seen = {im.shape[:2] for s in scenes for im in s[7]["textures"]["images"]}
        assert (1, 1) in shapes_seen and (4, 5) in shapes_seen
        assert not hostile or any(s[7]["textures"]["rejected"] is not None for s in scenes)
    if name == "shapes_only":
        assert all(len(FS.shape_blocks(s[0])) > 3 for s in scenes if len(s[0]) > 12)  # several block groups
        assert sum(len(FS.shape_blocks(s[0])) > 3 for s in scenes) >= len(scenes) * 3 // 4


@pytest.mark.parametrize("hostile", [False, True])
def test_near_misses_cover_every_edit(hostile):
    scenes = lane_scenes("near_miss", hostile)
    count = {}
    for s in scenes:
        count[s[7]["edit"]] = count.get(s[7]["edit"], 0) + 1
        base = s[7]["base"]
        assert s[6][0] != base and s[6][0] in (FS.GENERAL, FS.PPS_SPECULAR)  # it left its class
    assert sorted(count) == sorted(FS.NEAR_MISS_KINDS) and len(count) == 10
    assert min(count.values()) >= 5, count
    whats = {s[7]["what"] for s in scenes}
    for w in ("unknown_type/front", "unknown_type/middle", "unknown_type/end"):
        assert w in whats, whats
    both = {s[7]["what"] for hh in (False, True) for s in lane_scenes("near_miss", hh)}
    for w in ("count/11", "count/13", "count/12+plane", "count/5", "count/7"):
        assert w in both, both
    assert any(s[6][0] == FS.PPS_SPECULAR for s in scenes)  # ... and the other PPS class is among the targets


def library_flags(mats):
    """material_flags() from the LIBRARY's thresholds (srt_bernoulli_threshold_host)"""
    thr = {k: [T.bernoulli_threshold_host(m[k]) for m in mats] for k in ("metallic", "specular", "transmittance")}
    unit = all(t < (1 << 32) for ts in thr.values() for t in ts)
    plain = all(FS.is_plain(c) for m in mats for c in m["color"])
    return unit, unit and plain and all(t == 0 for t in thr["specular"])


@pytest.mark.parametrize("name,hostile", CASES)
def test_restatement_agrees_with_the_librarys_thresholds(name, hostile):
    for shapes, tris, mats, *_ in lane_scenes(name, hostile):
        assert FS.material_flags(mats) == library_flags(mats)
        for m in mats[:8]:
            for k in ("metallic", "specular", "transmittance"):
                assert FS.threshold_by_definition(m[k]) == T.bernoulli_threshold_host(m[k])


def test_restatement_on_the_hand_built_scenes():
    """the ten scenes of tests/test_gpu_scene_class.py, whose classes the GPU suite asserts against the library"""
    import test_gpu_scene_class as SC
    for name in SC.SCENES:
        shapes, tris, mats, cls = SC.scene(name)
        assert FS.expected_class(shapes, mats, SC.options()) == cls, name
    shapes, tris, mats, cls = SC.scene("base")
    assert FS.expected_class(shapes, mats, SC.options(bounces=0)) == FS.GENERAL
    assert FS.expected_class(shapes, mats, SC.options(show_normals=True)) == FS.GENERAL
    assert FS.expected_class(shapes, mats, SC.options(), textured=True) == FS.GENERAL
    assert FS.expected_class(shapes, mats, SC.options(), count_tris=True) == FS.GENERAL
    # the LDS border: 7 shapes hold 65 materials, 12 spheres 62
    pad = lambda n: R.concat(R.MATERIAL, mats, np.zeros(n - len(mats), R.MATERIAL))
    assert FS.expected_class(shapes, pad(65), SC.options()) == FS.PPS and FS.expected_class(shapes, pad(66), SC.options()) == FS.GENERAL
    s12 = SC.scene("spheres12")[0]
    assert FS.expected_class(s12, pad(62), SC.options()) == FS.SSS and FS.expected_class(s12, pad(63), SC.options()) == FS.GENERAL


HOSTILE_SAMPLE = 40


@pytest.mark.parametrize("name", list(FS.LANES))
def test_hostile_scenes_still_show_something(name, sky, oracle):
    """40 hostile scenes per lane through the oracle: at most a quarter have more than half their pixels NaN or exactly the
    sky's value (the same dispatch over no shapes at all); in the class lanes paths bounce (rays > paths)"""
    scenes = lane_scenes(name, True)
    sample = len(scenes) if name.startswith("texvar_") else HOSTILE_SAMPLE  # (the texvar lanes run 20 scenes: all of them, same share)
    assert len(scenes) >= sample
    blank, rays, paths = 0, 0, 0
    for shapes, tris, mats, cam, rd, sd, expected, extra in scenes[:sample]:
        with np.errstate(all="ignore"):
            want, oc = oracle.render(rd, sd, shapes, tris, mats, sky, counters=True, nthreads=4)
            empty_sd = sd.copy()
            empty_sd["num_shapes"] = 0
            nothing = oracle.render(rd, empty_sd, shapes[:0], tris, mats, sky, nthreads=4)
        nan = np.isnan(want[..., :3]).any(axis=-1)
        only_sky = (want.view(np.uint32) == nothing.view(np.uint32)).all(axis=-1)
        if (nan | only_sky).mean() > 0.5:
            blank += 1
        rays, paths = rays + oc["rays"], paths + oc["paths"]
    print(f"{name}: {blank} of {sample} hostile scenes mostly NaN or sky; rays {rays}, paths {paths}")
    assert blank <= sample // 4, (name, blank)
    if name in FS.CLASS_LANES:
        assert rays > paths, (name, rays, paths)
