"""The wave-wide ("w9") field forms at their documented operand bounds -- TEST INFRASTRUCTURE ONLY.

og_hook_w9_raw_d (hooks build, owshen_amd/csrc/field_ops.hip) hands one routine of field_w9.hip.h / mimc7.hip.h its operands as raw
limbs, one 64-lane workgroup per case, and returns the result word of all 64 lanes.  The same cases run through the CPU interpreter
(tests/test_emu_w9_raw.py), where the cross-lane reads are rendezvous and the inline assembly is not compiled, and on the hardware
(tests/test_gpu_w9_raw.py), where they are DPP moves, v_permlane16_swap and the hand-scheduled v_and_b32_dpp.

References, zero tolerance:
  * strict product (29-bit digit): the VALUE (a b + ((-a b / N) mod 2^261) N) / 2^261, whatever the limbs of a and b are;
  * lazy product (32-bit digit): the lane model below -- sixteen 64-bit accumulators walked exactly as the header describes, every
    one asserted below 2^64 -- plus, independently of it, the residue a b 2^-261 mod N and the bound a b / 2^261 + 8.01 N.
    (An integer CIOS loop whose digit is taken from the low 32 bits of the WHOLE accumulator is not this product: lane 0 sees only
    its own column in bits 29 .. 31, so the digits agree mod 2^29 only and the values differ by multiples of N.)
  * w9_carry, w9_sub + w9_carry, the spread / collect seam: integer identities on the limbs;
  * one MiMC7 round: the lane model per product, all five outputs of both rows, below the bounds table of mimc7.hip.h;
  * the two-to-one hash: oracle/py/mimc7.
Limbs below 2^29 + 32 after a product and 2^29 + 8 after a carry, and every lane outside the nine (2 x 9) limbs zero."""
import ctypes as C
import functools
import random

import numpy as np

from oracle.py import fields, mimc7

MASK, M32, RR = (1 << 29) - 1, (1 << 32) - 1, 1 << 261
MODS = {0: fields.R, 1: fields.P}
FIELD_NAMES = {0: "Fr", 1: "Fq"}
SLOTS, OUTS = 3, 5
OPS = {"mul": 0, "mul_rows": 1, "mul_rows_lazy": 2, "carry": 3, "sub4": 4, "sub8": 5, "sub16": 6, "seam": 7, "round": 8, "hash": 9}
FIELDS = {"mul": (0, 1), "mul_rows": (0, 1), "mul_rows_lazy": (0, 1), "carry": (0, 1), "sub4": (1,), "sub8": (1,), "sub16": (1,),
          "seam": (0, 1), "round": (0,), "hash": (0,)}
PARAMS = [(name, f) for name in OPS for f in FIELDS[name]]
LIMB_CEIL = (1 << 31) - 1              # both operands of a product (field_w9.hip.h)
T_CEIL = (1 << 31) + (1 << 9) - 1      # the round's t = x + k + c (mimc7.hip.h)
# the bounds table of w9_mimc7_round<2>, in hundredths of N: t < 21 in; t^2, t^3, t^4, t^6, t^7 out
ROUND_BOUNDS = {"t2": 1070, "t3": 940, "t4": 870, "t6": 860, "t7": 850}


def limbs(v):
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & MASK for i in range(9)]


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def pushed(v, ceil, rnd=None):
    """limbs of v with carries pushed DOWN: limb i + k 2^29, limb i + 1 - k -- as far as `ceil` allows, or a random part of that"""
    l = limbs(v)
    for i in range(8):
        k = min(l[i + 1], (ceil - l[i]) >> 29)
        if rnd is not None:
            k = rnd.randrange(k + 1)
        l[i] += k << 29
        l[i + 1] -= k
    assert value(l) == v and all(0 <= x <= ceil for x in l)
    return l


@functools.lru_cache(None)
def _nl(N):
    return limbs(N) + [0]


@functools.lru_cache(None)
def inv29(N):
    return (-pow(N, -1, 1 << 29)) % (1 << 29)   # FqParams::INV / FrParams::INV: 29 bits, also where the digit keeps 32


@functools.lru_cache(None)
def _ninv(N):
    return pow(N, -1, RR)


def strict_value(a, b, N):
    ab = a * b
    return (ab + ((-ab * _ninv(N)) % RR) * N) >> 261


def lane_mul(a, b, N, lazy):
    """w9_mul on one row of sixteen lanes: a = nine uniform limbs, b = nine spread limbs; -> nine result limbs.  Every accumulator
    is asserted below 2^64, every word below 2^32."""
    nl, bl, inv = _nl(N), list(b) + [0], inv29(N)       # lanes 9 .. 15 hold b = N = 0: their accumulators stay zero
    acc = [0] * 10
    mm = M32 if lazy else MASK
    for ai in a:
        acc = [x + ai * y for x, y in zip(acc, bl)]
        m = ((acc[0] & M32) * inv) & mm
        acc = [x + m * y for x, y in zip(acc, nl)]
        assert max(acc) < 1 << 64, "a 64-bit accumulator overflows"
        assert acc[0] & MASK == 0
        acc = [(x >> 29) + (y & MASK) for x, y in zip(acc, acc[1:] + [0])]
    assert max(acc) >> 29 <= M32 and acc[9] == 0
    out = [(acc[j] & MASK) + ((acc[j - 1] >> 29) if j else 0) for j in range(9)]
    assert max(out) <= M32
    return out


def round_model(t, N):
    """w9_mimc7_round<2>: -> {name: (row 0 limbs, row 1 limbs)} for t2, t4, t6, t6r0, x"""
    t2 = lane_mul(t, t, N, True)
    r0_t4, r1_t3 = lane_mul(t2, t2, N, True), lane_mul(t2, t, N, True)
    r0_t6, r1_t7 = lane_mul(r0_t4, t2, N, True), lane_mul(r0_t4, r1_t3, N, True)
    return {"t2": (t2, t2), "t4": (r0_t4, r1_t3), "t6": (r0_t6, r1_t7), "t6r0": (r0_t6, r0_t6), "x": (r1_t7, r1_t7)}


@functools.lru_cache(None)
def _round_constants(N):
    """the round constants as the context holds them: fe_to_mont of the canonical constant, a strict product by 2^522 mod N (its
    VALUE, below 2 N, not only its residue), normalized limbs"""
    return tuple(tuple(limbs(strict_value(c, RR * RR % N, N))) for c in mimc7.CONSTANTS)


def hash_model(l, r, N):
    """w9_mimc7_hash2<2> on limbs, every hard limit asserted on the way (the 64-bit accumulators inside lane_mul, limbs below 2^31 +
    2^9 into a round and below 2^32 into the carry, a b < 169 N^2 into the strict product, every value below 2^261) and the bounds
    table of mimc7.hip.h with them: t < 21 N, x < 8.5 N, k < 10.5 N; -> (normalized limbs of the result, the largest t / N in thousandths)"""
    consts, t_max = _round_constants(N), 0

    def rounds(x, k):
        nonlocal t_max
        for c in consts:
            t = [a + b + d for a, b, d in zip(x, k, c)]
            assert max(t) <= T_CEIL and value(t) < 21 * N, "t outside what a round takes"
            t_max = max(t_max, value(t) * 1000 // N)
            x = round_model(t, N)["x"][0]
            assert value(x) * 100 < ROUND_BOUNDS["t7"] * N
        return x
    k1 = [a + b for a, b in zip(l, rounds(l, [0] * 9))]
    assert value(k1) * 10 < 105 * N
    out = [2 * a + b + c for a, b, c in zip(k1, r, rounds(r, k1))]
    assert max(out) < (1 << 31) + (1 << 30) + 96 and value(out) * 10 < 315 * N and 315 * N < 10 * RR
    one = limbs(RR % N)
    assert value(one) * value(out) < 169 * N * N
    red = lane_mul(one, carry_model(out), N, False)
    assert value(red) == strict_value(value(one), value(out), N) < 2 * N
    return limbs(value(red)), t_max


def kn_limbs(N, K):
    """w9_kn_limb<M, K>: K N with two units borrowed into every limb below the top"""
    l = limbs(K * N)
    out = [l[0] + (2 << 29)] + [l[i] + (2 << 29) - 2 for i in range(1, 8)] + [l[8] - 2]
    assert value(out) == K * N
    return out


def carry_model(x):
    out = [(x[j] if j == 8 else x[j] & MASK) + ((x[j - 1] >> 29) if j else 0) for j in range(9)]
    assert max(out) <= M32, "the case itself overflows a word"
    return out


class Case:
    __slots__ = ("slots", "tag")

    def __init__(self, slots, tag):
        self.slots, self.tag = [list(s) for s in slots], tag


def _edge_values(N, top):
    return [0, 1, N - 1, N, 2 * N - 1, 13 * N, top - 1]


def _mul_cases(N, rnd, strict, ceil, top):
    """(a, b0, b1): b0 in row 0, b1 in row 1.  strict: every pair inside a b < 169 N^2 BY CONSTRUCTION (a partner above the bound is
    replaced by the largest admissible one, so the edge of the precondition is itself a case)"""
    edges = _edge_values(N, top)
    vals = edges + [rnd.randrange(top) for _ in range(10)] + [rnd.randrange(top - N, top) for _ in range(3)]
    lim = 169 * N * N

    def fit(a, b):
        if strict and a * b >= lim:
            b = (lim - 1) // a
            assert b < top and a * b < lim <= a * (b + 1)
        return b
    cases = []
    for a in vals:
        partners = edges + [rnd.choice(vals), rnd.randrange(top)]
        for k, b0 in enumerate(partners):
            b1 = partners[(k + 3) % len(partners)]
            b0, b1 = fit(a, b0), fit(a, b1)
            cases.append(Case([limbs(a), limbs(b0), limbs(b1)], ("norm", a, b0, b1)))
            cases.append(Case([pushed(a, ceil), pushed(b0, ceil), pushed(b1, ceil)], ("ceil", a, b0, b1)))
            cases.append(Case([pushed(a, ceil, rnd), pushed(b0, ceil, rnd), pushed(b1, ceil, rnd)], ("part", a, b0, b1)))
    if strict:   # the pairs that sit ON the precondition: a b = 169 N^2 - (less than a)
        assert sum(1 for c in cases if lim - c.tag[1] * c.tag[2] <= c.tag[1] and c.tag[1]) >= 9
    return cases


@functools.lru_cache(None)
def table(name, field):
    N = MODS[field]
    rnd = random.Random(f"w9_raw/{name}/{field}")
    if name in ("mul", "mul_rows"):
        return tuple(_mul_cases(N, rnd, True, LIMB_CEIL, 21 * N))
    if name == "mul_rows_lazy":
        return tuple(_mul_cases(N, rnd, False, T_CEIL, 21 * N))
    if name == "carry":
        cases = []
        rows = [[0] * 9, [M32] * 8 + [M32 - 7], [MASK] * 9, [1 << 29] * 9, [M32] + [0] * 8, [0] * 7 + [M32, 0]]
        rows += [[rnd.randrange(1 << 32) for _ in range(8)] + [rnd.randrange((1 << 32) - 8)] for _ in range(40)]
        for k, r in enumerate(rows):
            cases.append(Case([r, rows[(k + 1) % len(rows)]], ("limbs",)))
        return tuple(cases)
    if name.startswith("sub"):
        K = int(name[3:])
        # minuends: what the group law hands in (a product below 2 N, S below 1.2 N) and the table's largest coordinates beside them
        mins = [0, 1, N - 1, N, 2 * N - 1, 93 * N // 10 - 1, 172 * N // 10 - 1] + [rnd.randrange(2 * N) for _ in range(8)]
        subs = [0, 1, N - 1, N, (K - 2) * N - 1] + [rnd.randrange((K - 2) * N) for _ in range(6)] + [rnd.randrange((K - 3) * N, (K - 2) * N) for _ in range(3)]
        cases = []
        for a in mins:
            for b in subs:
                cases.append(Case([limbs(a), limbs(b)], ("norm", a, b)))
                cases.append(Case([pushed(a, LIMB_CEIL), pushed(b, (1 << 30) - 3)], ("ceil", a, b)))
                cases.append(Case([pushed(a, LIMB_CEIL, rnd), pushed(b, (1 << 30) - 3, rnd)], ("part", a, b)))
        return tuple(cases)
    if name == "seam":
        vals = [0, 1, N - 1, N, 2 * N - 1, 21 * N - 1, RR - 1, (1 << 253) - 1] + [rnd.randrange(RR) for _ in range(12)]
        return tuple(Case([l], (form, v)) for v in vals for form, l in (("norm", limbs(v)), ("ceil", pushed(v, M32)), ("part", pushed(v, M32, rnd))))
    if name == "round":
        vals = [0, 1, N - 1, N, 2 * N - 1, 20 * N - 1, 21 * N - 1, 20 * N, 19 * N] + [rnd.randrange(19 * N, 21 * N) for _ in range(24)] + \
               [rnd.randrange(21 * N) for _ in range(8)]
        return tuple(Case([l], (form, v)) for v in vals for form, l in (("norm", limbs(v)), ("ceil", pushed(v, T_CEIL)), ("part", pushed(v, T_CEIL, rnd))))
    if name == "hash":
        vs = [0, 1, N - 1, rnd.randrange(N), rnd.randrange(N)]
        pairs = [(vs[0], vs[0]), (vs[1], vs[2]), (vs[2], vs[2]), (vs[3], vs[4])]
        cases = []
        for k, (l, r) in enumerate(pairs):
            for jl, jr in ((0, 0), (1, 1), (0, 1), (1, 0)) if k in (2, 3) else ((0, 0), (1, 1)):
                cases.append(Case([limbs(l + jl * N), limbs(r + jr * N)], (l, r, jl, jr)))
        return tuple(cases)
    raise KeyError(name)


def _rows(word):
    """the 64 lanes of one result word -> (row 0 limbs, row 1 limbs, everything else)"""
    w = [int(x) for x in word]
    return w[0:9], w[16:25], w[9:16] + w[25:64]


def check(name, field, cases, got):
    """got: n x OUTS x 64 words"""
    N = MODS[field]
    assert len(got) == len(cases)
    counted = {"product_limb_max": 0, "carry_limb_max": 0}
    for k, (c, g) in enumerate(zip(cases, got)):
        where = f"{name} {FIELD_NAMES[field]} case {k} {c.tag[:1]}"
        r0, r1, rest = _rows(g[0])
        if name in ("mul", "mul_rows", "mul_rows_lazy"):
            a, b0, b1 = (value(s) for s in c.slots)
            assert (a, b0, b1) == tuple(c.tag[1:])
            assert not any(rest), f"{where}: a lane outside the limbs is not zero"
            rows = ((b0, c.slots[1], r0),) if name == "mul" else ((b0, c.slots[1], r0), (b1, c.slots[2], r1))
            if name == "mul":
                assert not any(r1), f"{where}: row 1 is not zero"
            for b, bl, r in rows:
                assert max(r) < (1 << 29) + 32, f"{where}: limb above 2^29 + 32: {r}"
                counted["product_limb_max"] = max(counted["product_limb_max"], max(r))
                v = value(r)
                assert v % N == a * b * pow(RR, -1, N) % N, f"{where}: wrong residue"
                if name == "mul_rows_lazy":
                    assert r == lane_mul(c.slots[0], bl, N, True), f"{where}: not the lane model's limbs"
                    assert v * 100 < (a * b * 100 >> 261) + 801 * N, f"{where}: above a b / 2^261 + 8.01 N"
                else:
                    assert a * b < 169 * N * N
                    assert v == strict_value(a, b, N), f"{where}: value {v} is not the strict product's"
                    assert v < (a * b >> 261) + N + 1 and v < 2 * N
                    assert r == lane_mul(c.slots[0], bl, N, False), f"{where}: not the lane model's limbs"
        elif name == "carry":
            assert not any(rest), f"{where}: a lane outside the limbs is not zero"
            for x, r in ((c.slots[0], r0), (c.slots[1], r1)):
                assert r == carry_model(x), f"{where}: {r}"
                assert value(r) == value(x) and max(r[:8]) < (1 << 29) + 8
                counted["carry_limb_max"] = max(counted["carry_limb_max"], max(r[:8]))
        elif name.startswith("sub"):
            K = int(name[3:])
            a, b = value(c.slots[0]), value(c.slots[1])
            assert b < (K - 2) * N and max(c.slots[1]) <= (1 << 30) - 3
            ck = kn_limbs(N, K)
            raw = [c.slots[0][j] + ck[j] - c.slots[1][j] for j in range(9)]
            assert min(raw) >= 0 and max(raw) <= M32, f"{where}: the model itself borrows or overflows"
            assert not any(rest) and not any(r1), f"{where}: a lane outside the limbs is not zero"
            assert r0 == carry_model(raw), f"{where}: {r0}"
            assert value(r0) == a - b + K * N, f"{where}: not a - b + {K} N"
            assert max(r0[:8]) < (1 << 29) + 8
            counted["carry_limb_max"] = max(counted["carry_limb_max"], max(r0[:8]))
        elif name == "seam":
            v = value(c.slots[0])
            assert r0 == c.slots[0] and not any(r1) and not any(rest), f"{where}: spread"
            w = [int(x) for x in g[1]]
            for row in range(4):
                assert w[16 * row:16 * row + 9] == limbs(v), f"{where}: row {row} collected {w[16 * row:16 * row + 9]}"
                assert not any(w[16 * row + 9:16 * row + 16])
        elif name == "round":
            t = c.slots[0]
            assert value(t) < 21 * N and max(t) <= T_CEIL
            want = round_model(t, N)
            for o, key in enumerate(("t2", "t4", "t6", "t6r0", "x")):
                q0, q1, rest = _rows(g[o])
                assert not any(rest), f"{where}: {key}: a lane outside the limbs is not zero"
                assert (q0, q1) == want[key], f"{where}: {key} differs from the lane model"
                assert max(q0 + q1) < (1 << 29) + 32
            tv = value(t)
            rinv = pow(RR, -1, N)
            mont = lambda *f: functools.reduce(lambda x, y: x * y * rinv % N, f)
            t2, t3 = mont(tv, tv), mont(tv, tv, tv)
            t4 = mont(t2, t2)
            powers = {"t2": t2, "t3": t3, "t4": t4, "t6": mont(t4, t2), "t7": mont(t4, t3)}
            seen = {"t2": want["t2"][0], "t3": want["t4"][1], "t4": want["t4"][0], "t6": want["t6"][0], "t7": want["x"][0]}
            for key, l in seen.items():
                assert value(l) % N == powers[key], f"{where}: {key}: wrong residue"
                assert value(l) * 100 < ROUND_BOUNDS[key] * N, f"{where}: {key} = {value(l) * 100 // N / 100} N, above the table"
                counted[key] = max(counted.get(key, 0), value(l) * 1000 // N)
        elif name == "hash":
            l, r, jl, jr = c.tag
            rinv = pow(RR, -1, N)
            want = mimc7.hash2(l * rinv % N, r * rinv % N) * RR % N
            w = [int(x) for x in g[0]]
            for row in range(4):
                got_l = w[16 * row:16 * row + 9]
                assert max(got_l) <= MASK and not any(w[16 * row + 9:16 * row + 16]), f"{where}: row {row}: limbs not normalized"
                assert value(got_l) < 2 * N and value(got_l) % N == want, f"{where}: row {row}: wrong hash"
            assert all(w[16 * row:16 * row + 9] == w[:9] for row in range(4))
            model, t_max = hash_model(c.slots[0], c.slots[1], N)
            assert w[:9] == model, f"{where}: the residue is the oracle's, the value is not the lane model's"
            counted["t_max"] = max(counted.get("t_max", 0), t_max)
    return counted


def pack(cases):
    arr = np.zeros((len(cases), SLOTS, 9), dtype=np.uint32)
    for k, c in enumerate(cases):
        arr[k, :len(c.slots)] = np.array(c.slots, dtype=np.uint64).astype(np.uint32)
    return arr


def run(ctx, name, field, stride=1):
    """one upload, ONE call of og_hook_w9_raw_d (one launch of n one-wave workgroups), one download.  stride > 1 takes every
    stride-th case (the CPU interpreter's hash cases); returns (cases run, figures seen)"""
    cases = table(name, field)[::stride]
    fn = ctx._lib.og_hook_w9_raw_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    d_in = ctx.to_device(pack(cases))
    d_out = ctx.empty(len(cases) * OUTS * 64 * 4)
    ctx._pre()
    ctx._check(fn(ctx._h, field, OPS[name], ctx.ptr(d_in), len(cases), ctx.ptr(d_out)))
    got = np.asarray(ctx.to_host(d_out)).view(np.uint32).reshape(len(cases), OUTS, 64)
    return len(cases), check(name, field, cases, got.tolist())
