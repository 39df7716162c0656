"""CPU: the texture sampler on the images, coordinates and scenes of tests/texture_edge_cases.py. The C oracle
(oracle/srt_oracle.c sample_texture under albedo) equals the numpy restatement of the rule (tests/texture_ref.py) bit for bit
on every pair of every image, through orc_sample_texture, through the guide buffer and through the two-bounce canvas; the
crafted route really hands the sampler u = v = 1.0f; the set reads every column and row as first and as second tap, wraps in
both directions and trips the guard from either axis and either sign; at least nine in ten of the targeted grid coordinates
land on their target to the bit; and each mutant of the rule moves texels, so a device sampler with that slip cannot pass
tests/test_gpu_texture_edges.py. Every comparison is exact (NaN equals NaN)."""
import numpy as np
import pytest

import texture_edge_cases as EC
import texture_ref as TR
from conftest import bits_equal

F = np.float32
IMAGES = EC.images()
DEEP = EC.deep_set(IMAGES)
PAIRS = {(name, filt): EC.pairs(IMAGES[name], filt) for name in IMAGES for filt in EC.FILTERS}
W, H = EC.FRAME
N = W * H


def moved(a, b):
    """rows whose bits differ (NaN equal to NaN)"""
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


def texels(name, filt, ps=None, mutant=None):
    su, sv = EC.pair_scales(PAIRS[name, filt] if ps is None else ps)
    if mutant is None:
        return TR.sample(IMAGES[name], filt, su, sv)
    return EC.mutant_sample([IMAGES[name]], 0, filt, su, sv, mutant)


def test_images_are_what_they_say():
    assert [IMAGES[f"{w}x{h}"].shape for w, h in EC.SIZES] == [(h, w, 4) for w, h in EC.SIZES]
    for name in EC.PLAIN:
        img = IMAGES[name]
        assert len(np.unique(img)) == img.size and img.min() >= 0 and img.max() < 4, name  # alpha equals no colour value
    assert IMAGES["16384x1"].nbytes == 256 * 1024
    na = IMAGES["3x2_nan_alpha"]
    assert np.isnan(na[..., 3]).all() and np.array_equal(na[..., :3], IMAGES["3x2"][..., :3])
    sp = IMAGES["specials"]
    assert sp[0, 0, 0] == F(-1.75) and np.signbit(sp[0, 1, 0]) and sp[0, 1, 0] == 0 and 0 < sp[1, 3, 1] < np.finfo(F).tiny
    assert sp[2, 4, 2] == F(1e30) and np.isposinf(sp[2, 2, :3]).all() and np.isnan(sp[1, 1, :3]).all()
    assert np.isfinite(sp[..., :3]).sum() == sp[..., :3].size - 6
    assert len(DEEP) == EC.MAX_TEXTURES and DEEP[0].shape == (3, 4099, 4) and DEEP[-1] is IMAGES[EC.DEEP_IMAGE]
    off = EC.texel_offset(DEEP, EC.MAX_TEXTURES - 1)
    assert off > 30000 and off % 2 == 1, off


# ---- the crafted route does what it claims -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", EC.ROUTES)
@pytest.mark.parametrize("axis", list(EC.CRAFTED))
def test_crafted_hits_have_uv_one(oracle, axis, route):
    """At the one ray of a crafted scene the UV before the scale is (1.0f, 1.0f) to the bit, in every pixel, and the plane is what
    the ray hits: a property of the case, no tolerance."""
    scn, cam, _ = EC.crafted_scene(axis, route)
    rd, sd = EC.render_data(cam, 0.0, W, H), EC.scene_data(len(scn[0]))
    u, v, hit, _ = EC.hit_uvs(oracle, rd, sd, (scn[0][:1], scn[1], scn[2]))
    assert hit.all()
    one = np.ones(N, F)
    assert bits_equal(u, one) and bits_equal(v, one), (axis, u[:3], v[:3])
    ph = oracle.primary_hits(rd, sd, *scn, np.arange(N), np.zeros(N, np.int32))
    assert (ph["material"] == 0).all() and len(np.unique(ph["dir"].view(np.uint32) & 0x7FFFFFFF, axis=0)) == 1


# ---- oracle against restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", list(IMAGES))
def test_oracle_sampler_equals_the_restatement(oracle, name, filt):
    """orc_sample_texture at u = v = 1 under each pair's scales, texture_ref.sample, and the module's own statement of the rule
    (the one the mutants are slips of) agree on every pair."""
    ps = PAIRS[name, filt]
    want = texels(name, filt)
    one = np.ones(1, F)
    got = np.concatenate([oracle.sample_texture(IMAGES[name], filt, one, one, p["su"], p["sv"]) for p in ps])
    assert bits_equal(got, want), (name, filt, moved(got, want))
    assert bits_equal(EC.mutant_sample([IMAGES[name]], 0, filt, *EC.pair_scales(ps)), want)


def oracle_frames(oracle, sky, scn, cam, image_set, index, filt, ps, fov=0.0, w=W, h=H, uvs=None):
    """per pair: the oracle's guide (h * w, 4) and two-bounce canvas (h * w, 4)"""
    shapes, tris, mats = scn
    rd, sd = EC.render_data(cam, fov, w, h), EC.scene_data(len(shapes))
    table = EC.oracle_table(scn, image_set, EC.binding(len(mats), index, filt, 1.0, 1.0), uvs)
    out = []
    for p in ps:
        table.bindings[0]["scale_u"], table.bindings[0]["scale_v"] = p["su"], p["sv"]
        _, ah = oracle.features_textured(rd, sd, shapes, tris, mats, table, 1)
        with np.errstate(all="ignore"):
            canvas = oracle.render_textured(rd, sd, shapes, tris, mats, sky, table)
        out.append((ah.reshape(-1, 4), canvas.reshape(-1, 4)))
    return out


def white_radiance(oracle, sky, scn, cam, fov=0.0, w=W, h=H):
    shapes, tris, mats = scn
    rd, sd = EC.render_data(cam, fov, w, h), EC.scene_data(len(shapes))
    ids = np.arange(w * h, dtype=np.int32)
    return oracle.trace_paths(rd, sd, shapes, tris, mats, sky, ids, np.zeros_like(ids)).astype(F)


@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", list(IMAGES))
def test_oracle_frames_equal_the_restatement_on_the_z_plane(oracle, sky, name, filt):
    """The full list on the z plane: the guide is the restatement's texel in every pixel with a hit count of 1, the canvas is texel
    * the untextured oracle's white radiance of the same path (one multiply per channel; 1 sample, so / 1) for every finite texel."""
    scn, cam, _ = EC.crafted_scene("z")
    ps = PAIRS[name, filt]
    want = texels(name, filt)
    L = white_radiance(oracle, sky, scn, cam)
    assert (L > 0).all()  # every pixel's bounce ends in the sky: the canvas shows the texel
    for p, tex, (ah, canvas) in zip(ps, want, oracle_frames(oracle, sky, scn, cam, [IMAGES[name]], 0, filt, ps)):
        assert bits_equal(ah[:, :3], np.tile(F(0) + tex, (N, 1))) and (ah[:, 3] == 1).all(), (name, filt, p["name"])  # (0 + texel: the guide is a sum)
        if np.isfinite(tex).all():  # (a texel that is not finite meets a 0 somewhere in the path's sums: the oracle's canvas is the statement)
            assert bits_equal(canvas[:, :3], F(0) + (tex[None, :] * L).astype(F)), (name, filt, p["name"])  # (the canvas, too, is a sum from 0)


@pytest.mark.parametrize("route", EC.ROUTES)
@pytest.mark.parametrize("axis", list(EC.CRAFTED))
def test_oracle_frames_equal_the_restatement_on_every_route(oracle, sky, axis, route):
    """The subset (integers, half-integers, the guard) on every orientation and route, images 3x2, 7x1 and 4099x3."""
    scn, cam, _ = EC.crafted_scene(axis, route)
    L = white_radiance(oracle, sky, scn, cam)
    for name in ("3x2", "7x1", "4099x3"):
        for filt in EC.FILTERS:
            ps = EC.pairs(IMAGES[name], filt, subset=True)
            want = texels(name, filt, ps)
            for p, tex, (ah, canvas) in zip(ps, want, oracle_frames(oracle, sky, scn, cam, [IMAGES[name]], 0, filt, ps)):
                assert bits_equal(ah[:, :3], np.tile(F(0) + tex, (N, 1))) and (ah[:, 3] == 1).all(), (axis, route, name, filt, p["name"])
                assert bits_equal(canvas[:, :3], F(0) + (tex[None, :] * L).astype(F)), (axis, route, name, filt, p["name"])


@pytest.mark.parametrize("filt", EC.FILTERS)
def test_deep_set_reads_the_last_image(oracle, sky, filt):
    """Bound as image 63 of the deep set the image under test gives what it gives alone, in the oracle and in the restatement."""
    name = EC.DEEP_IMAGE
    scn, cam, _ = EC.crafted_scene("z")
    ps = EC.pairs(IMAGES[name], filt, subset=True)
    want = texels(name, filt, ps)
    assert bits_equal(EC.mutant_sample(DEEP, EC.MAX_TEXTURES - 1, filt, *EC.pair_scales(ps)), want)
    alone = oracle_frames(oracle, sky, scn, cam, [IMAGES[name]], 0, filt, ps)
    deep = oracle_frames(oracle, sky, scn, cam, DEEP, EC.MAX_TEXTURES - 1, filt, ps)
    for tex, a, d in zip(want, alone, deep):
        assert bits_equal(a[0], d[0]) and bits_equal(a[1], d[1]) and bits_equal(d[0][:, :3], np.tile(F(0) + tex, (N, 1)))


# ---- the compared scenes ------------------------------------------------------------------------------------------------------------
def compared_frames(oracle, case, filt):
    """[(rd, sd, u, v, hit, tri)] per camera of a compared case"""
    out = []
    for cam, fov, w, h in case["cams"]:
        rd, sd = EC.render_data(cam, fov, w, h), EC.scene_data(len(case["scn"][0]))
        uvs = case["uvs"](filt) if case["uvs"] else None
        out.append((rd, sd, *EC.hit_uvs(oracle, rd, sd, case["scn"], uvs)))
    return out


@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", ["tilted", "sphere", "sphere_tall", "mesh"])
def test_compared_scenes_equal_the_restatement(oracle, sky, name, filt):
    """Tilted plane, sphere and mesh: the oracle's guide is texture_ref.sample at texture_ref's UV of the oracle's primary hit."""
    case = EC.compared_cases(IMAGES)[name]
    shapes, tris, mats = case["scn"]
    uvs = case["uvs"](filt) if case["uvs"] else None
    table = EC.oracle_table(case["scn"], [case["image"]], EC.binding(1, 0, filt, *case["scale"]), uvs)
    hits = 0
    for rd, sd, u, v, hit, _ in compared_frames(oracle, case, filt):
        want = np.where(hit[:, None], TR.sample(case["image"], filt, u, v, *case["scale"]), F(1))  # (a miss counts albedo 1)
        _, ah = oracle.features_textured(rd, sd, shapes, tris, mats, table, 1)
        assert bits_equal(ah[..., :3].reshape(-1, 3), want), (name, filt)
        assert np.array_equal(ah[..., 3].reshape(-1) == 1, hit)
        hits += int(hit.sum())
    assert hits > 300


@pytest.mark.parametrize("filt", EC.FILTERS)
def test_sphere_cameras_meet_poles_and_seam(oracle, filt):
    """The fixed cameras put v on 0 and 1 (the poles: rows 0 and H wrapped) and u on both ends of [0, 1] at the seam."""
    case = EC.compared_cases(IMAGES)["sphere"]
    frames = dict(zip(EC.SPHERE_TARGETS, compared_frames(oracle, case, filt)))
    for name, (_, _, u, v, hit, _) in frames.items():
        assert hit.all(), name
    assert set(frames["at_+y"][3].tolist()) == {1.0} and set(frames["at_-y"][3].tolist()) == {0.0}
    seam_u = np.concatenate([frames[c][2] for c in EC.SPHERE_TARGETS if c.startswith("at_-x")])
    assert seam_u.min() < 1e-6 and seam_u.max() > 1 - 1e-6
    assert set(frames["at_+x"][2].tolist()) == {0.5}


@pytest.mark.parametrize("filt", EC.FILTERS)
def test_mesh_hits_both_sides_of_each_seam_and_every_guard(oracle, filt):
    """Per seam triangle the interpolated coordinate lands below and above the seam it names, on both axes (floor(pu) takes
    both values); per guard triangle the guard fires, from the axis its corner is on, in at least 20 pixels."""
    case = EC.compared_cases(IMAGES)["mesh"]
    image = case["image"]
    sides = {k: [set(), set()] for k in ("seam_a", "seam_b")}
    fired = {k: 0 for k in EC.MESH_TRIANGLES[2:]}
    for rd, sd, u, v, hit, tri in compared_frames(oracle, case, filt):
        fp = EC.footprint(image, filt, u, v)
        for k, name in enumerate(EC.MESH_TRIANGLES):
            sel = hit & (tri == k)
            if k < 2:
                with np.errstate(all="ignore"):
                    sides[name][0] |= set(np.floor(fp["fu"][sel]).tolist())
                    sides[name][1] |= set(np.floor(fp["fv"][sel]).tolist())
            else:
                bad = ~fp["okv"][sel] & fp["oku"][sel] if name.endswith("_v") else ~fp["oku"][sel] & fp["okv"][sel]
                fired[name] += int(bad.sum())
    print(sides, fired)
    assert sides["seam_a"] == [{0.0, 1.0}, {0.0, 1.0}] and sides["seam_b"] == [{2.0, 3.0}, {1.0, 2.0}], sides
    assert min(fired.values()) >= 20, fired


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", list(IMAGES))
def test_coverage(name, filt):
    """Per image and filter, over its pairs: every column and row of a small axis is read as i0 and (LINEAR) as i1; the wrap
    occurs in both directions (a tap pair W-1 -> 0, and a negative coordinate that reads W-1), on the seams of a long axis too;
    the guard fires from u alone, from v alone, from +2^30 and from -2^30 on either axis, and not at the float just below."""
    image = IMAGES[name]
    Himg, Wimg = image.shape[:2]
    ps = PAIRS[name, filt]
    fp = EC.footprint(image, filt, *EC.pair_scales(ps))
    ok = fp["ok"]
    for n, k0, k1, f in ((Wimg, "i0", "i1", "fu"), (Himg, "j0", "j1", "fv")):
        cols = set(range(n)) if n <= EC.SMALL_SIDE else {0, 1, n - 2, n - 1}
        assert cols <= set(fp[k0][ok].tolist()), (name, filt, k0)
        assert (cols if n <= EC.SMALL_SIDE else {0, 1, n - 1}) <= set(fp[k1][ok].tolist()), (name, filt, k1)
        if filt == EC.LINEAR:
            assert ((fp[k0] == n - 1) & (fp[k1] == 0) & ok).any(), (name, filt, "wrap up")
        assert ((fp[f] < 0) & (fp[k0] == n - 1) & ok).any(), (name, filt, "wrap down")
        assert ((fp[f] >= n) & (fp[k0] == 0) & ok).any(), (name, filt, "wrap past the end")
    assert (~fp["oku"] & fp["okv"]).any() and (fp["oku"] & ~fp["okv"]).any()  # from u alone, from v alone
    for f in ("fu", "fv"):
        v = fp[f]
        for edge in (EC.TWO30, -EC.TWO30):
            assert (v == edge).any(), (name, filt, f, edge)
        for edge in (EC.BELOW30, -EC.BELOW30):
            assert ((v == edge) & ok).any(), (name, filt, f, edge)  # just below: the guard lets it through, with the other axis ordinary
        assert np.isinf(v).any() or min(Wimg, Himg) == 1
    # at the guard's own values with the other axis ordinary, the texel is texel (0, 0) -- and just below it is the wrapped one
    tex = texels(name, filt)
    for p, t, good in zip(ps, tex, ok):
        e = p["u"] if p["v"] is None else p["v"] if p["u"] is None else None
        if e is not None and e["label"] in ("+2^30", "-2^30"):
            assert not good and bits_equal(t, image[0, 0, :3]), (name, filt, p["name"])


# ---- exact landing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", EC.FILTERS)
@pytest.mark.parametrize("name", list(IMAGES))
def test_targets_land(name, filt):
    """The targeted texel-grid coordinates -- every integer, half-integer and guard value of both axes -- are hit to the bit by the
    scale the search found (nine in ten is the demand; all of them land), checked with the rule alone: the sampler's coordinate
    of the entry's scale is recomputed here. The floats NEXT to a grid coordinate cannot all be reached (scale * fN steps over
    floats, and x - 0.5 is finer than x): those that miss are exactly the names the module lists per axis size, and each of them
    still lies strictly on its own side of the grid coordinate, within 4 floats of it (of the product before the - 0.5; next to 0, within N denormals)."""
    Himg, Wimg = IMAGES[name].shape[:2]
    total = landed = every = every_landed = 0
    for n in (Wimg, Himg):
        missed = []
        for e in EC.axis_entries(n, filt):
            if e["kind"] == "overflow":
                continue
            value = EC.grid_value(e["scale"], n, filt)
            hit = bool(EC.same_bits(value, e["target"]))
            assert hit == e["landed"]
            every, every_landed = every + 1, every_landed + hit
            if e["kind"] in ("grid", "guard"):
                total, landed = total + 1, landed + hit
            if not hit:
                missed.append(e["label"])
            if e["kind"] == "near":
                side = -1 if e["label"][-1] == "-" else 1
                assert (value - e["anchor"]) * side > 0, (name, filt, n, e["label"], value)
                step = np.spacing(F(abs(e["anchor"]) + (0.5 if filt == EC.LINEAR else 0)))
                reach = max(4 * np.float64(step), n * np.float64(EC.DENORMAL))  # (next to 0 the products are multiples of N denormals)
                assert abs(np.float64(value) - np.float64(e["anchor"])) <= reach, (name, filt, n, e["label"], value)
        assert missed == EC.CANNOT_LAND[n, filt], (name, filt, n, missed)
    print(name, filt, "grid and guard", landed, "of", total, "all", every_landed, "of", every)
    assert landed * 10 >= total * 9 and landed == total, (name, filt, landed, total)


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def test_mutants_move_texels():
    """Texels (of the pairs of all images, both filters; for offset_ignored, of the deep set's subset) that a slip of the rule moves:
    see MUTANT_COUNTS below, asserted. Every mutant moves texels on at least one image."""
    counts = {}
    for m in EC.MUTANTS:
        if m == "offset_ignored":
            n = 0
            for filt in EC.FILTERS:
                ps = EC.pairs(IMAGES[EC.DEEP_IMAGE], filt, subset=True)
                su, sv = EC.pair_scales(ps)
                n += moved(EC.mutant_sample(DEEP, EC.MAX_TEXTURES - 1, filt, su, sv, m), EC.mutant_sample(DEEP, EC.MAX_TEXTURES - 1, filt, su, sv))
            counts[m] = {"deep": n}
        else:
            counts[m] = {name: sum(moved(texels(name, filt, mutant=m), texels(name, filt)) for filt in EC.FILTERS) for name in EC.PLAIN + ["3x2_nan_alpha"]}
        print(f"{m:16s}", counts[m])
        assert max(counts[m].values()) > 0, m
    totals = {m: sum(c.values()) for m, c in counts.items()}
    print(totals)
    assert totals == MUTANT_COUNTS


# texels moved, summed over the plain images and the NaN-alpha one, both filters (offset_ignored: over the deep set's subset); the
# same figures stand in texture_edge_cases.MUTANTS beside each slip
MUTANT_COUNTS = {"trunc": 575, "wrap_no_add": 222, "clamp_second": 437, "stride_h": 1333, "guard_le": 120, "guard_u_only": 108, "guard_wrapped": 186,
                 "alpha_blue": 3072, "offset_ignored": 110, "no_half": 1289, "nearest_round": 465}


def test_nan_alpha_never_reaches_the_colour():
    for filt in EC.FILTERS:
        assert bits_equal(texels("3x2_nan_alpha", filt), texels("3x2", filt))
        assert not np.isnan(texels("3x2_nan_alpha", filt)).any()


def test_specials_are_read():
    """Each special texel comes out as stored under NEAREST (-0 keeps its sign), and most LINEAR texels stay finite."""
    tex = texels("specials", EC.NEAREST)
    for value in EC.SPECIAL_TEXELS.values():
        same = np.isnan(tex[:, 0]) if np.isnan(value) else (tex[:, 0].view(np.uint32) == F(value).view(np.uint32))
        assert same.any(), value
    lin = texels("specials", EC.LINEAR)
    assert np.isfinite(lin).all(axis=1).mean() > 0.5 and not np.isfinite(lin).all()
