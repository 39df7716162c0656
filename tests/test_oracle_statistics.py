"""CPU: are detmath's built-ins (cos / log / pow / atan2pi as FMA polynomials, dot / cross / mix fused, normalize
through a Newton rsqrt) UNBIASED, not just inside the OpenCL ULP bounds? A path tracer is chaotic, so renders made with
different realisations of the built-ins cannot be compared bit for bit -- but they must agree as statistics.

Both sides are the reference's own render.cl compiled for x86-64 (oracle/Makefile `ref`): once with detmath behind the
built-ins (oracle/_ref/libsrt_ref.so, what the goldens come from), once with glibc's libm and textbook unfused vector
helpers (libsrt_ref_libm.so). For every golden scene, at a raised sample count:
  * the image means agree within Monte-Carlo error,
  * the RMS difference between the two images is no larger than the RMS difference between two renders of ONE
    implementation with different seeds (the noise floor): there is no systematic per-pixel offset either.
Where oracle/_ref is not built, the detmath side is the port (bit-identical to libsrt_ref.so: tests/golden/make_golden.py
--ref-checks asserts it on these very renders) and the libm side is libsrt_ref_libm.so's renders stored in
tests/golden/ref_checks.npz."""
import numpy as np
import pytest

import cases as C
import golden_io
from oracle import oracle_py


@pytest.fixture(scope="module")
def sides(oracle):
    """(detmath side, libm side): live builds where oracle/_ref has them, else the port and the stored libm renders."""
    det = oracle_py.Oracle("ref") if oracle_py.ref_available() else oracle
    if oracle_py.ref_libm_available():
        libm = oracle_py.Oracle("ref_libm")
        return det, lambda name, case, sky: C.stats_render(libm, case, sky, C.STATS_SEEDS[0])
    stored = golden_io.load_ref_checks()
    return det, lambda name, case, sky: stored[f"libm/{name}"]


def _stats(img):
    return np.nan_to_num(img.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)  # NaN-poisoned pixels carry no statistics


@pytest.mark.parametrize("name", sorted(C.build_cases()))
def test_detmath_built_ins_agree_with_libm_statistically(name, sides, sky):
    det, libm = sides
    case = C.build_cases()[name]
    if bool(case["rd"]["show_normals"]):
        pytest.skip("show_normals images carry no Monte-Carlo noise: covered bit for bit by the goldens")
    a = _stats(C.stats_render(det, case, sky, C.STATS_SEEDS[0]))
    b = _stats(libm(name, case, sky))
    a2 = _stats(C.stats_render(det, case, sky, C.STATS_SEEDS[1]))  # same implementation, other seeds: the noise floor
    clip = lambda x: np.minimum(x, 4.0)  # fireflies (a few paths into the sun lobe) would dominate every RMS otherwise
    a, b, a2 = clip(a), clip(b), clip(a2)
    mean_a, mean_b = a.mean(), b.mean()
    noise = np.sqrt(((a - a2) ** 2).mean())
    diff = np.sqrt(((a - b) ** 2).mean())
    n = a.size
    # means: difference below 5 standard errors of the difference of two noisy means (plus 0.1 % for exactly-empty scenes)
    assert abs(mean_a - mean_b) <= 5.0 * noise / np.sqrt(n) + 1e-3 * max(mean_a, 1e-6), (name, mean_a, mean_b, noise)
    # per-pixel: same implementation / other seeds differ as much as the two implementations do
    assert diff <= 1.25 * noise + 1e-6, (name, diff, noise)
