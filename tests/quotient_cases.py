"""Inputs of the quotient (h_poly) tests shared by the CPU interpreter (tests/test_emu_kernels.py) and the GPU
(tests/test_gpu_quotient_shapes.py) -- TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from oracle.py import fields

RM1 = np.frombuffer((fields.R - 1).to_bytes(32, "little"), dtype=np.uint8)


def rand_fr_np(rng, *shape):
    a = rng.integers(0, 256, (*shape, 32), dtype=np.uint8)
    a[..., 31] &= 0x1F  # < 2^253 < r
    return a


def extreme_triples(d):
    """the (a, b, c) that maximise every intermediate sum of k_ntt_block4's lazy butterflies: all r - 1, alternating 0 / r - 1, all 1"""
    full, alt, ones = np.tile(RM1, (d, 1)), np.tile(RM1, (d, 1)), np.zeros((d, 32), np.uint8)
    alt[::2] = 0
    ones[:, 0] = 1
    return ((full, full, full), (alt, full, ones), (ones, alt, full), (full, alt[::-1].copy(), alt))


def block_shape_inputs(log_d, seed_base=40):
    """seeded random evaluations with the extreme values 0, 1, r - 1 riding along"""
    d = 1 << log_d
    rng = np.random.default_rng(seed_base + log_d)
    a, b, c = (rand_fr_np(rng, d) for _ in range(3))
    a[0] = RM1
    b[-1] = RM1
    c[d // 2] = RM1
    if d >= 4:
        a[1] = 0
        b[2] = 0
        b[2, 0] = 1
        c[3] = RM1
        a[3] = RM1
        b[3] = RM1
    return a, b, c


@functools.lru_cache(None)
def block_shape_oracle(log_d):
    """the C restatement's quotient of block_shape_inputs(log_d), computed once per session (2^21 costs the host seconds)"""
    from oracle.c import binding as oc
    h = oc.h_poly(*block_shape_inputs(log_d))
    h.setflags(write=False)
    return h
