"""PCG-RXS-M-XS-32 backwards (a plain module, not a test module): the seed whose k-th draw returns a chosen output.

The generator (tests/test_oracle_features.py `_rand`, the oracle's random_float): the state steps s <- s * A + C, then the
output is a permutation of the NEW state: w = (s >> ((s >> 28) + 4)) ^ s, r = w * M, out = (r >> 22) ^ r. Every stage is a
bijection of the 32-bit words -- A and M are odd, an xor with a right shift of itself keeps the top bits it is made from --
so each has an inverse, and a draw can be aimed: at 0 (random_float = 0, -2 log u = +inf), or at one of the 128 largest
outputs, which the conversion to float rounds to 2^32 (random_float = 1, -2 log u = -0)."""
import numpy as np

A, C_, M = 747796405, 2891336453, 277803737
MASK = 0xFFFFFFFF
A_INV, M_INV = pow(A, -1, 1 << 32), pow(M, -1, 1 << 32)


def step(s):
    """the state after one more draw (s: int or uint32 array)"""
    if isinstance(s, np.ndarray):
        return ((s.astype(np.uint64) * A + C_) & MASK).astype(np.uint32)
    return (int(s) * A + C_) & MASK


def output(s):
    """the draw made from state s (the state AFTER its step)"""
    s = np.asarray(s, np.uint32).astype(np.uint64)
    r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(M)) & np.uint64(MASK)
    return (((r >> np.uint64(22)) ^ r) & np.uint64(MASK)).astype(np.uint32)


def draws(seed, n):
    """the first n draws from seed, and the state they leave"""
    out, s = [], int(seed)
    for _ in range(n):
        s = step(s)
        out.append(int(output(s)))
    return out, s


def state_of_output(out):
    """the state whose draw is `out`"""
    out = int(out) & MASK
    r = out ^ (out >> 22)  # the shift is more than half the word: one round undoes it
    w = (r * M_INV) & MASK
    shift = (w >> 28) + 4  # the top four bits of s pass through unchanged (shift >= 4)
    s, known = w, shift  # the top `known` bits of s are right; each round fixes `shift` more
    while known < 32:
        s = w ^ (s >> shift)
        known += shift
    return s & MASK


def seed_for(out, draw):
    """the seed whose draw number `draw` (1 = the first) returns `out`"""
    s = state_of_output(out)
    for _ in range(draw):
        s = ((s - C_) * A_INV) & MASK
    return s
