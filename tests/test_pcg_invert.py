"""CPU: tests/pcg_invert.py against the generator's own definition (the oracle's random_float): a seed aimed at an output
at a draw returns it there, for the outputs the trace kernel's wave votes are about (0, the 128 largest) and random ones."""
import numpy as np
import pytest

import pcg_invert as P

F32 = np.float32


def test_forward_model_is_the_oracles_generator(oracle):
    rng = np.random.RandomState(5)
    for seed in [0, 1, 0xFFFFFFFF] + [int(v) for v in rng.randint(0, 1 << 32, size=20, dtype=np.uint64)]:
        got, state = P.draws(seed, 8)
        want, want_state = oracle.random_floats(seed, 8)
        assert state == want_state
        assert np.array_equal((np.array(got, np.uint32).astype(F32) / F32(4294967296.0)).view(np.uint32), want.view(np.uint32))


def test_output_permutation_is_inverted():
    rng = np.random.RandomState(6)
    outs = [0, 1, 2, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE, 0xFFFFFFFF, 0x80000000, 0x0FFFFFFF, 0xF0000000]
    outs += [int(v) for v in rng.randint(0, 1 << 32, size=4000, dtype=np.uint64)]
    states = np.array([P.state_of_output(o) for o in outs], np.uint32)
    assert np.array_equal(P.output(states), np.array(outs, np.uint32))


@pytest.mark.parametrize("draw", [1, 2, 3, 4, 5, 6])
def test_aimed_seeds_draw_zero_and_one(oracle, draw):
    """count 0 -> random_float 0; each of the 128 largest outputs -> random_float 1; the 129th largest does not"""
    for out, want in [(0, 0.0)] + [(v, 1.0) for v in (0xFFFFFF80, 0xFFFFFFC1, 0xFFFFFFFF)]:
        seed = P.seed_for(out, draw)
        assert P.draws(seed, draw)[0][-1] == out
        assert oracle.random_floats(seed, draw)[0][-1] == F32(want)
    u = oracle.random_floats(P.seed_for(0xFFFFFF7F, draw), draw)[0][-1]
    assert u < F32(1.0) and u == F32(1.0) - F32(2.0 ** -24)
