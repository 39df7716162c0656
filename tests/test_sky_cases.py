"""CPU: the sky lookup on the skies and cameras of tests/sky_cases.py. The C oracle (oracle/srt_oracle.c sky_box) equals the numpy
restatement of the rule (tests/sky_ref.py) bit for bit on every frame; the set reaches every side of the clamp and every
footprint along the seam and the poles; each mutant of the restatement moves pixels, so a device sampler with that slip cannot
pass tests/test_gpu_sky_edges.py; an alpha lane of NaN changes nothing; and the reference build's own sky_box, stored in
tests/golden/ref_checks.npz, is the oracle's on the exact directions. Every comparison is exact (NaN equals NaN)."""
import numpy as np
import pytest

import golden_io
import sky_cases as SC
import sky_ref as SR
from conftest import bits_equal

SKIES = SC.skies()
CAMERAS = SC.cameras()


@pytest.fixture(scope="module")
def dirs(oracle):
    """(camera, frame) -> (w * h, 3) directions: computed once, shared, never changed"""
    out = {(c, f): SC.directions(oracle, *CAMERAS[c], *f) for c in CAMERAS for f in SC.FRAMES}
    for d in out.values():
        d.flags.writeable = False
    return out


@pytest.fixture(scope="module")
def frames(oracle):
    """(sky, camera, frame) -> the oracle's 1-sample empty-scene frame, x, y, z: (w * h, 3)"""
    out = {}
    for s, sky in SKIES.items():
        for c in CAMERAS:
            for f in SC.FRAMES:
                out[s, c, f] = SC.oracle_frame(oracle, sky, *CAMERAS[c], *f)[..., :3].reshape(-1, 3).copy()
                out[s, c, f].flags.writeable = False
    return out


def moved(a, b):
    """pixels whose bits differ (NaN equal to NaN)"""
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


def test_skies_are_what_they_say():
    assert [SKIES[f"{w}x{h}"].shape for w, h in SC.SIZES] == [(h, w, 4) for w, h in SC.SIZES]
    for name in SC.FINITE:
        rgb = SKIES[name][..., :3]
        assert len(np.unique(rgb)) == rgb.size and rgb.min() >= 0 and rgb.max() < 4, name
        assert rgb.size < 30 or rgb.max() > 3, name  # HDR: values above 1
        assert np.all(SKIES[name][..., 3] == 1)
    for name in ("5x7_nan_alpha", "3x2_nan_alpha"):
        assert np.isnan(SKIES[name][..., 3]).all() and np.array_equal(SKIES[name][..., :3], SKIES[name[:3]][..., :3])
    sp = SKIES["specials"]
    assert np.signbit(sp[0, 0, 0]) and sp[0, 0, 0] == 0 and 0 < sp[6, 4, 1] < np.finfo(np.float32).tiny and sp[3, 2, 2] < 0
    assert sp[3, 0, 0] == np.float32(1e30) and np.isposinf(sp[2, 1, :3]).all() and np.isnan(sp[5, 3, :3]).all()
    assert np.isfinite(sp[..., :3]).sum() == sp[..., :3].size - 6


@pytest.mark.parametrize("sky_name", list(SKIES))
def test_oracle_equals_the_restatement(sky_name, dirs, frames):
    """The oracle's 1-sample frame of an empty scene, sun off, is the restatement's sky_box + 0 of the same directions, bit for bit,
    for every camera and both frame sizes."""
    sd = SC.scene_data()
    for (c, f), d in dirs.items():
        assert bits_equal(SR.frame(sd, SKIES[sky_name], d), frames[sky_name, c, f]), (sky_name, c, f)


@pytest.mark.parametrize("sky_name", ["3x2", "31x13", "specials"])
def test_oracle_sky_box_equals_the_restatement(sky_name, oracle, dirs):
    """The same directions through Oracle.sky_box (no camera, no canvas), sun off; and once with the sun on, whose lobe the
    restatement states for the default integer focus."""
    sky = SKIES[sky_name]
    d = np.concatenate([dirs[c, SC.FRAMES[0]][::7] for c in CAMERAS] + [SC.random_directions()])
    for sun in (False, True) if sky_name == "3x2" else (False,):
        sd = SC.scene_data(sun)
        with np.errstate(all="ignore"):
            want = np.asarray([oracle.sky_box(sd, sky, x) for x in d], np.float32)
        got = SR.sky_box(sd, sky, d)
        assert bits_equal(got, want), (sky_name, sun)
        if sun:
            assert moved(got, SR.sky_box(SC.scene_data(False), sky, d)) > 100  # (the lobe is in the comparison)


def npairs(n):
    return 1 if n == 1 else n + 1  # (0, 0), (0, 1), .. (n - 2, n - 1), (n - 1, n - 1)


# distinct (i0, i1) pairs the frames reach on the clamped rows of the 4099 x 3 sky, of 2 * 4100: 1073 pixels a frame cannot
# hold them all; the two ends at the seam on both rows are demanded by name
WIDE_POLE_PAIRS = 3000


def test_coverage(dirs):
    """Per sky, over its cameras (directions with a NaN left out), pixels of all frames:

      sky      x0 < 0  x0+1 > W-1  y0 < 0  y0+1 > H-1   footprints: seam columns   pole rows
      1x1       10903    24076     11965    23014                    1 of 1          1 of 1
      1x5       10903    24076      5631     5622                    6 of 6          2 of 2
      7x1        5117    10570     11965    23014                    2 of 2          8 of 8
      3x2        7074    12501      7182     7188                    6 of 6          8 of 8
      5x7        5605    11007      5238     5229                   16 of 16        12 of 12
      31x13      4316     9865      2666     2666                   28 of 28        64 of 64
      4099x3     4127     9677      5953     5944                    8 of 8       3416 of 8200 (see WIDE_POLE_PAIRS)

    A footprint is (i0, i1, j0, j1) after the clamp; a seam column is i0 == i1 (0 or W - 1: the clamp in x), a pole row j0 == j1.
    Every side of the clamp is reached on every sky, every footprint the size allows along them on every sky but the widest,
    and the seam camera's u runs over both ends."""
    for name in SC.FINITE:
        sky = SKIES[name]
        H, W = sky.shape[:2]
        sides = np.zeros(4, np.int64)
        seam, pole = set(), set()
        for (c, f), d in dirs.items():
            fp = SR.footprint(sky, d[~np.isnan(d).any(axis=1)])
            sides += [(fp["x0"] < 0).sum(), (fp["x0"] + 1 > W - 1).sum(), (fp["y0"] < 0).sum(), (fp["y0"] + 1 > H - 1).sum()]
            quad = np.stack([fp[k] for k in ("i0", "i1", "j0", "j1")], axis=1)
            seam |= {tuple(q) for q in quad[(quad[:, 0] == quad[:, 1]) & ((fp["x0"] < 0) | (fp["x0"] + 1 > W - 1))].tolist()}
            pole |= {tuple(q) for q in quad[(quad[:, 2] == quad[:, 3]) & ((fp["y0"] < 0) | (fp["y0"] + 1 > H - 1))].tolist()}
        print(name, sides.tolist(), len(seam), len(pole))
        assert sides.min() > 0, (name, sides)
        assert len(seam) == (1 if W == 1 else 2) * npairs(H), (name, sorted(seam))
        if name == "4099x3":
            assert len(pole) >= WIDE_POLE_PAIRS, len(pole)
            assert {(0, 0, 0, 0), (W - 1, W - 1, 0, 0), (0, 0, H - 1, H - 1), (W - 1, W - 1, H - 1, H - 1)} <= pole
        else:
            assert len(pole) == (1 if H == 1 else 2) * npairs(W), (name, sorted(pole))
    for f in SC.FRAMES:  # the seam camera: both ends of u, exactly, and pixels clamped on either side on an image 31 wide
        fp = SR.footprint(SKIES["31x13"], dirs["seam", f])
        assert fp["u"].min() < 1 / 62 and fp["u"].max() > 1 - 1 / 62 and (fp["x0"] < 0).sum() > 10 and (fp["x0"] + 1 > 30).sum() > 10
        fixed = np.concatenate([SR.footprint(SKIES["31x13"], dirs[c, f])["u"] for c in ("at_-x_z+0", "at_-x_z-0")])
        assert fixed.min() == 0.0 and fixed.max() == 1.0
    # the zero direction: u in {0, 0.5, 1} by the signs of its zeros, v = 0.5
    for c, us in (("at_zero", {0.0, 0.5}), ("at_zero_u1", {0.5, 1.0})):
        fp = SR.footprint(SKIES["5x7"], dirs[c, SC.FRAMES[0]])
        assert not dirs[c, SC.FRAMES[0]].any() and set(fp["u"].tolist()) == us and set(fp["v"].tolist()) == {0.5}, c
    assert np.isnan(dirs["at_nan", SC.FRAMES[0]]).any(axis=1).all()


def test_mutants_move_pixels(dirs, frames):
    """Pixels (of 34,979 per sky: the 19 cameras without a NaN, both frames) that a slip of the rule moves, per finite sky:

      mutant              1x1    1x5    7x1    3x2    5x7  31x13  4099x3
      repeat                0  11253  15687  27467  22717  19465  22018    wraps at the seam and the poles instead of clamping
      clamp_to_w        21473  19157  18871  17608  14678  12518  14237    clamps to W (H), one texel past the row (image)
      a_from_clamped     5120   9075   7798  10262   6421   4970   6191    the fraction of the clamped coordinate: 0 at an edge, not 0.5
      round             13162  15556  16312  17032  16994  16963  17012    rint for floor
      truncate          13162  11683  13334  13099  10217   6971   9623    trunc for floor: differs below 0
      scale_w_minus_1    5120  30181  30175  34048  34404  34971  34522    u * (W - 1)
      w10_w01_swapped    4640  22317  15311  26182  27617  30337  28072
      rows_flipped          0  22092      0  22092  22092  22092  22092    row 0 taken for the top
      xy_swapped            0      0      0  27132  28186  30346  28529    texel (i, j) read at i * H + j
      alpha_added       34979  34979  34979  34979  34979  34979  34979

    Every mutant moves pixels on at least one finite sky (most on every sky on which it is a different rule at all)."""
    sd = SC.scene_data()
    table = {}
    for m in SR.MUTANTS:
        table[m] = {name: sum(moved(SR.frame(sd, SKIES[name], d, m), frames[name, c, f]) for (c, f), d in dirs.items()) for name in SC.FINITE}
        print(f"{m:18s}" + "".join(f"{table[m][name]:7d}" for name in SC.FINITE))
        assert max(table[m].values()) > 0, m
    for m in ("clamp_to_w", "a_from_clamped", "round", "truncate", "scale_w_minus_1", "w10_w01_swapped", "alpha_added"):
        assert min(table[m].values()) > 0, (m, table[m])
    for m, same in (("repeat", ["1x1"]), ("rows_flipped", ["1x1", "7x1"]), ("xy_swapped", ["1x1", "1x5", "7x1"])):
        assert all((table[m][name] == 0) == (name in same) for name in SC.FINITE), (m, table[m])
    # wrapping and the clamp to W are caught ON the edge: by the fixed cameras at the seam alone, on the widest image too
    # (a_from_clamped is the same number there but for rounding: the moving cameras catch it)
    for m in ("repeat", "clamp_to_w"):
        for name in ("3x2", "4099x3"):
            n = sum(moved(SR.frame(sd, SKIES[name], dirs[c, f], m), frames[name, c, f]) for c in ("at_-x_z+0", "at_-x_z-0") for f in SC.FRAMES)
            assert n > 0, (m, name)


@pytest.mark.parametrize("name", ["5x7", "3x2"])
def test_nan_alpha_never_reaches_the_colour(name, frames):
    for c in CAMERAS:
        for f in SC.FRAMES:
            assert bits_equal(frames[f"{name}_nan_alpha", c, f], frames[name, c, f]), (name, c, f)


def test_specials_sky_leaves_most_pixels_finite(frames):
    """-0, a denormal, a negative value, 1e30, +inf and NaN as texels: over this file's frames of the specials sky at least half of
    the pixels stay finite and at least one does not (32,054 of 36,820 are finite); so it is on the moving cameras alone (no NaN direction), and the
    negative texel and 1e30 are seen."""
    every = np.concatenate([frames["specials", c, f] for c in CAMERAS for f in SC.FRAMES])
    finite = np.isfinite(every).all(axis=1)
    print("specials: finite pixels", int(finite.sum()), "of", len(every))
    assert finite.sum() * 2 >= len(every) and not finite.all()
    moving = np.concatenate([frames["specials", c, f] for c in SC.MOVING for f in SC.FRAMES])
    fin = np.isfinite(moving).all(axis=1)
    assert fin.sum() * 2 >= len(moving) and not fin.all()
    assert (moving[fin] < 0).any() and (moving[fin] > 1e28).any()
    # the corner texel of -0 and the sun's + 0: the seam's low corner (-0 in all four taps) is +0, never -0
    low = frames["specials", "at_-x_y-2", SC.FRAMES[0]]
    assert (low == 0).any() and not np.signbit(low[low == 0]).any()
    plain = np.concatenate([frames["5x7", c, f] for c in SC.MOVING for f in SC.FRAMES])
    assert moved(moving, plain) > len(moving) // 4


def test_reference_build_agrees_on_the_exact_directions(oracle, ref):
    """render.cl's own sky_box (compiled for x86-64, sun on) on the fov_scale = 0 directions -- the poles, the seam with z = +0, -0,
    +-1e-7, +x, the zero vector, NaN -- and 200 random ones, over the 3x2, 5x7 and specials skies: its stored results
    (tests/golden/ref_checks.npz "sky/*", make_golden.py --ref-checks) are the oracle's, and so are the live build's where
    oracle/_ref is built. This pins the reference's u, v mapping at the seam and the poles and its sun lobe. It proves nothing
    about the filter: the reference build's read_imagef is the shim's (oracle/cl_builtins_shim.cpp), the same text as the
    oracle's sampler; the filter's independent statement is tests/sky_ref.py."""
    stored = golden_io.load_ref_checks()
    d = stored["sky/dirs"]
    assert bits_equal(d, SC.ref_check_directions(oracle)) and len(d) > 200 + 12
    sd = SC.scene_data(sun=True)
    for name in SC.REF_CHECK_SKIES:
        with np.errstate(all="ignore"):
            got = np.asarray([oracle.sky_box(sd, SKIES[name], x) for x in d], np.float32)
        assert bits_equal(got, stored[f"sky/{name}"]), name
        assert bits_equal(got, SR.sky_box(sd, SKIES[name], d)), name
        if ref is not None:
            assert bits_equal(got, np.asarray([ref.sky_box(sd, SKIES[name], x) for x in d], np.float32)), name
