"""CPU: the identity behind the diffuse waves of the NO_SPEC scene classes (DESIGN.md 5 "Diffuse waves"; device_shading.h "DIFFUSE
WAVES") and a numpy restatement of their operand guard.

On a plain diffuse lane the bounce comes to dir = fma(rough_dir - random_dir, +0, random_dir). The product of anything finite with
+0 is an exact +-0, so in float32 `x + (y - x) * 0` IS that fma, rounding for rounding. It is x, bit for bit, unless x is a zero
(+0 + -0 = +0) or y - x is not finite (NaN). The guard admits a lane when the smallest |random_dir component| is above 0 and the
sum of the ten magnitudes (random_dir, dir, nrm, smoothness) is at most 2^20. Checked here: whenever the guard admits an operand
set the identity holds through the whole chain reflect3 -> mix3 -> mix3, and every exception the design lists is refused.

The chain's other fmas (dot3, the first mix3) are formed as float32(float64 product + float64 addend): a double rounding that can
differ from the device's single one by an ulp, which cannot matter for what is asked of them here -- whether rough_dir - random_dir
is finite -- since the guard keeps every intermediate below 2^87."""
import numpy as np

F = np.float32
LIMIT = F(2.0 ** 20)


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def fma32(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def guard(random_dir, d, n, s):
    """diffuse_operands_ok: v_min3 skips NaNs (np.fmin); the sum runs in the kernel's order, in float32"""
    r, d, n, s = (np.abs(np.asarray(v, F)) for v in (random_dir, d, n, s))
    with np.errstate(all="ignore"):
        mn = np.fmin(np.fmin(r[..., 0], r[..., 1]), r[..., 2])
        sm = r[..., 0] + r[..., 1]
        for t in (r[..., 2], d[..., 0], d[..., 1], d[..., 2], n[..., 0], n[..., 1], n[..., 2], s):
            sm = (sm + t).astype(F)
        return (mn > 0) & (sm <= LIMIT)


def bounce_dir(random_dir, d, n, s):
    """the per-lane form of a plain diffuse lane: -> (new dir, rough_dir - random_dir)"""
    random_dir, d, n, s = (np.asarray(v, F) for v in (random_dir, d, n, s))
    with np.errstate(all="ignore"):
        dot = fma32(d[..., 2], n[..., 2], fma32(d[..., 1], n[..., 1], d[..., 0] * n[..., 0]))
        refl = d - n * (F(2) * dot)[..., None]
        rough = fma32(refl - random_dir, s[..., None], random_dir)
        diff = (rough - random_dir).astype(F)
        return (random_dir + diff * F(0)).astype(F), diff  # = fma(diff, +0, random_dir): the product is exact


def identity_holds(random_dir, d, n, s):
    out, _ = bounce_dir(random_dir, d, n, s)
    return (bits(out) == bits(random_dir)).all(axis=-1)


def test_scalar_identity_and_its_exceptions():
    """x + (y - x) * 0 == x bit for bit for finite y - x and x not a zero; not for x = -0, nor for y - x = inf, -inf, NaN or overflowing"""
    rng = np.random.RandomState(1)
    x = (rng.normal(size=100000) * 2.0 ** rng.randint(-120, 100, 100000)).astype(F)
    y = (rng.normal(size=100000) * 2.0 ** rng.randint(-120, 100, 100000)).astype(F)
    x = x[x != 0]
    y = y[:len(x)]
    with np.errstate(all="ignore"):
        assert np.isfinite(y - x).all()
        assert (bits(x + (y - x) * F(0)) == bits(x)).all()
        den = F(np.finfo(F).smallest_subnormal)
        for v in (den, -den, F(1e-40), F(3e38)):  # denormals and the largest magnitudes keep their bits
            assert bits(v + (F(1) - v) * F(0)) == bits(v)
        assert bits(F(-0.0) + (F(1) - F(-0.0)) * F(0)) != bits(F(-0.0))  # -0 + +0 = +0
        assert bits(F(0.0) + (F(1) - F(0.0)) * F(-1) * F(0)) == bits(F(0.0))  # (+0 survives either sign of the product; the guard refuses it all the same)
        for diff in (F(np.inf), F(-np.inf), F(np.nan), F(3e38) - F(-3e38)):
            assert np.isnan(F(0.5) + diff * F(0))


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(F)


def test_guard_admits_only_where_the_identity_holds():
    """10^5 random operand sets over a wide range of magnitudes: admitted => the bounce's dir is random_dir, and rough - random finite"""
    rng = np.random.RandomState(2)
    n = 100000
    scale = lambda lo, hi: (2.0 ** rng.uniform(lo, hi, (n, 1))).astype(F)
    r, d, nr = unit(rng, n) * scale(-40, 22), unit(rng, n) * scale(-10, 22), unit(rng, n) * scale(-10, 22)
    s = (rng.normal(size=n) * 2.0 ** rng.uniform(-30, 22, n)).astype(F)
    r[rng.rand(n) < 0.02, int(rng.randint(3))] = F(0.0)
    r[rng.rand(n) < 0.02, int(rng.randint(3))] = F(-0.0)
    s[rng.rand(n) < 0.02] = F(np.nan)
    ok = guard(r, d, nr, s)
    assert 0.2 * n < ok.sum() < 0.9 * n, ok.sum()  # both sides are populated
    out, diff = bounce_dir(r, d, nr, s)
    assert np.isfinite(diff[ok]).all()
    assert (bits(out[ok]) == bits(r[ok])).all()
    assert not ok[(r == 0).any(axis=1)].any() and not ok[np.isnan(s)].any()
    # unit vectors and a smoothness in [0, 1], as the kernel has them: everything without a zero component is admitted
    r, d, nr, s = unit(rng, n), unit(rng, n), unit(rng, n), rng.uniform(0, 1, n).astype(F)
    assert guard(r, d, nr, s).all() and identity_holds(r, d, nr, s).all()


BASE = dict(r=(0.36, -0.48, 0.8), d=(0.6, 0.0, -0.8), n=(0.0, 1.0, 0.0), s=0.5)
DEN = float(np.finfo(F).smallest_subnormal)
# name -> (operand edits, admitted?, the identity holds?) -- None: either (the guard is allowed to be stricter than the identity)
HOSTILE = {
    "tame": ({}, True, True),
    "random_dir_plus_zero": (dict(r=(0.6, 0.0, 0.8)), False, None),
    "random_dir_minus_zero": (dict(r=(0.6, -0.0, 0.8)), False, False),
    "random_dir_denormal": (dict(r=(0.6, DEN, 0.8)), True, True),
    "random_dir_nan": (dict(r=(np.nan, 0.6, 0.8)), False, None),
    "random_dir_all_nan": (dict(r=(np.nan, np.nan, np.nan)), False, None),
    "random_dir_inf": (dict(r=(np.inf, 0.6, 0.8)), False, False),
    "smoothness_0": (dict(s=0.0), True, True),
    "smoothness_minus_0": (dict(s=-0.0), True, True),
    "smoothness_1": (dict(s=1.0), True, True),
    "smoothness_denormal": (dict(s=DEN), True, True),
    "smoothness_2^19": (dict(s=2.0 ** 19), True, True),
    "smoothness_1e30": (dict(s=1e30), False, None),
    "smoothness_3e38_overflows_the_mix": (dict(s=3e38, d=(0.6, 0.5, -0.8)), False, False),
    "smoothness_inf": (dict(s=np.inf), False, False),
    "smoothness_nan": (dict(s=np.nan), False, False),
    "normal_0": (dict(n=(0.0, 0.0, 0.0)), True, True),
    "normal_1": (dict(n=(0.0, 0.0, 1.0)), True, True),
    "normal_2^19": (dict(n=(0.0, 2.0 ** 19, 0.0)), True, True),
    "normal_2^21": (dict(n=(0.0, 2.0 ** 21, 0.0)), False, None),
    "normal_1e20_overflows_reflect3": (dict(n=(0.0, 1e20, 0.0), d=(0.6, 0.5, -0.8)), False, False),
    "normal_nan": (dict(n=(np.nan, 1.0, 0.0)), False, False),
    "dir_inf": (dict(d=(np.inf, 0.0, -0.8)), False, False),
    "dir_nan": (dict(d=(0.6, np.nan, -0.8)), False, False),
    "dir_2^19": (dict(d=(2.0 ** 19, 0.0, -0.8)), True, True),
    "dir_1e25": (dict(d=(1e25, 0.5, -0.8)), False, None),
    "difference_overflows": (dict(d=(3e38, 3e38, 3e38), n=(1.0, 1.0, 1.0)), False, False),
}


def test_hostile_operands_on_both_sides_of_every_exception():
    for name, (edit, admitted, holds) in HOSTILE.items():
        o = {**BASE, **edit}
        r, d, n, s = np.array([o["r"]], F), np.array([o["d"]], F), np.array([o["n"]], F), np.array([o["s"]], F)
        got_ok, got_holds = bool(guard(r, d, n, s)[0]), bool(identity_holds(r, d, n, s)[0])
        assert got_ok == admitted, (name, got_ok)
        if holds is not None:
            assert got_holds == holds, (name, got_holds)
        assert got_holds or not got_ok, name  # admitted => the identity holds
