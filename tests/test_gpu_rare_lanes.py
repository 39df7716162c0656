"""GPU (MI355X): the bounce's wave-level votes. The scene classes' trace kernels decide the once-in-2^32 cases of a bounce
(a Box-Muller count of 0 or 2^32, a dot product of +-0 or NaN) with one vote per wave and run either the fast or the rare
form on ALL lanes. srt_selftest_rare_lanes runs those forms wave by wave next to the per-lane forms they replaced; here the
rare lanes sit nowhere, in one lane, in lane 0, in lane 63 and in all lanes of a wave, and the two must agree to the bit.
One small frame of the headline's scene class against the oracle guards the exec mask behind the new branches. (No
sphere-normal cases: that guard as one wave-level branch measured no gain and was not kept; div3_by_rcp is the
per-lane form it was, covered by srt_selftest_math out[8].)"""
import numpy as np
import pytest

import pcg_invert as P
from conftest import bits_equal
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
PLACEMENTS = {"none": [], "one": [17], "lane0": [0], "lane63": [63], "all": list(range(64))}


def bits(x):
    return int(np.array(x, F32).view(U32))


def waves_with(common_rows, rare_rows):
    """one wave per (rare row, placement): 64 lanes of rows drawn from common_rows (cycled), the placement's lanes replaced by
    the rare row. -> words [waves * 64, 8], rare mask [waves * 64]"""
    words, rare = [], []
    k = 0
    for row in rare_rows:
        for lanes in PLACEMENTS.values():
            w = np.zeros((64, 8), U32)
            for lane in range(64):
                w[lane, :len(common_rows[0])] = common_rows[k % len(common_rows)]
                k += 1
            m = np.zeros(64, bool)
            for lane in lanes:
                w[lane, :len(row)] = row
                m[lane] = True
            words.append(w)
            rare.append(m)
    return np.concatenate(words), np.concatenate(rare)


@pytest.fixture(scope="module")
def tr(T):
    t = T.Tracer(8, 8)
    yield t
    t.close()


def test_random_normal3_votes_on_count_0_and_2_pow_32(tr):
    """Seeds aimed (tests/pcg_invert.py) at an output of 0, one of the 128 largest, and their neighbours 1 and 2^32 - 129, at
    each of the six draws of a bounce's direction (draws 2, 4, 6 are the counts under the logarithm; 1, 3, 5 the angles, which
    need no vote)."""
    rng = np.random.RandomState(11)
    common = [[int(v)] for v in rng.randint(0, 1 << 32, size=997, dtype=np.uint64)]
    aimed = [(out, draw) for draw in (1, 2, 3, 4, 5, 6) for out in (0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFC1, 0xFFFFFFFF)]
    words, rare = waves_with(common, [[P.seed_for(out, draw)] for out, draw in aimed])
    # a few hundred plain waves behind them
    plain = np.zeros((200 * 64, 8), U32)
    plain[:, 0] = rng.randint(0, 1 << 32, size=len(plain), dtype=np.uint64)
    words = np.concatenate([words, plain])
    new, ref, bad = tr.selftest_rare_lanes(0, words)
    assert bad == 0 and np.array_equal(new, ref)
    # the generator has moved on by six draws, whichever form ran
    s = words[:, 0].copy()
    for _ in range(6):
        s = P.step(s)
    assert np.array_equal(new[:, 3], s)
    # and the rare values are what IEEE makes of them: u = 0 -> rho = +inf -> an infinite component (cos is never 0 at a float
    # angle); u = 1 -> rho = sqrt(-0) = -0 -> a zero component
    xyz = new[:, :3].view(F32)
    per_row = 64 * len(PLACEMENTS)
    for i, (out, draw) in enumerate(aimed):
        m = rare[i * per_row:(i + 1) * per_row]
        comp = xyz[i * per_row:(i + 1) * per_row, (draw - 1) // 2][m]
        assert len(comp) == 1 + 1 + 1 + 64
        if draw % 2 == 0 and out == 0:
            assert np.isinf(comp).all()
        elif draw % 2 == 0 and out >= 0xFFFFFF80:
            assert (comp == 0).all()
        else:
            assert np.isfinite(comp).all() and (comp != 0).all()


def test_sign_by_xor_votes_on_zero_and_nan_dots(tr):
    """Dots of +0, -0, NaN, +-denormal and +-inf among ordinary ones, over components that are ordinary, +-0, inf -- and NaN,
    which in the kernel always comes with a NaN dot (the dot product is taken WITH the vector): those rows carry one."""
    rng = np.random.RandomState(12)
    nan = bits(np.nan)
    ordinary = [[bits(v) for v in rng.normal(size=3)] + [bits(d)] for d in rng.normal(size=499)]
    dots = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, 1.0, -1.0]
    comps = [(0.3, -0.7, 0.2), (0.0, -0.0, 1.0), (-0.0, 0.0, -1.0), (np.inf, -np.inf, 1.0), (1e-40, -1e-40, 3e38)]
    rows = [[bits(c) for c in v] + [bits(d)] for d in dots for v in comps]
    rows += [[bits(c) for c in v] + [nan] for v in comps]  # a NaN dot over every kind of component
    rows += [[nan, bits(0.5), bits(-0.5), nan], [bits(0.5), nan | 0x80000000, bits(np.inf), nan | 0x80000000], [nan, nan, nan, 0x7F800001]]
    words, _ = waves_with(ordinary, rows)
    new, ref, bad = tr.selftest_rare_lanes(1, words)
    assert bad == 0 and np.array_equal(new, ref)
    # against the definition, independently of either device form: v * sign(d), sign(+-0) = +-0, sign(NaN) = 0
    v, d = words[:, :3].view(F32), words[:, 3].view(F32)
    with np.errstate(invalid="ignore"):
        sgn = np.where(d > 0, F32(1), np.where(d < 0, F32(-1), np.where(d == 0, d, F32(0)))).astype(F32)
        want = v * sgn[:, None]
    assert bits_equal(new[:, :3].view(F32), want)
    assert not new[:, 3].any()


def test_headline_class_frame_equals_oracle(T, sky, oracle):
    """64x32, 8 spp, 10 bounces of the sphere scene (the headline's scene class): canvas bits and counters."""
    shapes, tris, mats = S.sphere_scene()
    w, h = 64, 32
    t = T.Tracer(w, h)
    t.set_skybox(sky)
    t.options = R.render_data(w, h, 8, 10, camera_to_world=S.default_camera(), time=90125)
    t.scene_data = R.scene_data(len(shapes))
    t.update_scene(shapes, tris, mats)
    t.clear_canvas()
    t.reset_counters()
    t.trace()
    got, c = t.read_canvas(), t.counters()
    want, oc = oracle.render(t.options, t.scene_data, shapes, tris, mats, sky, counters=True)
    assert bits_equal(got, want)
    for k in ("paths", "rays", "sky", "nan_pixels"):
        assert c[k] == oc[k], (k, c, oc)
    assert c["watchdog"] == 0
    t.close()
