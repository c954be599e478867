"""One table of raw-limb cases for the 9 x 29-bit Montgomery layer (owshen_amd/csrc/field.hip.h, the Fq2 layer of ec.hip.h) with
a big-integer reference -- TEST INFRASTRUCTURE ONLY.

Three views of that layer answer to this table:
* the HOST column walk (MontCols), through og_hook_fe_raw_d of the CPU interpreter build (tests/test_emu_field_raw.py);
* the gfx950 asm TEXT executed on Python integers (tests/test_mont_asm.py);
* the asm on the HARDWARE, through og_hook_fe_raw_d of libowshen_gpu_hooks.so (tests/test_gpu_field_raw.py).

A case is up to eight operands given as limbs plus the name of the operand class every position holds.  Cases are BUILT to meet
the contract the routine documents (limb widths, at most one lazy operand per product, sum of products < 169 N^2, ...): every
op lists "profiles" -- one family of classes per operand position, chosen so that the worst members together still meet the
contract -- and for every profile, position and class of that position's family there are cases where THAT position holds THAT
class while the partners cycle through theirs.  The contract is asserted on every case before it is emitted; nothing is
skipped at run time.  Expected results are Python integers: for every Montgomery product form
    total = sum of products,  m = -total / N mod 2^261,  value = (total + m N) / 2^261 (+ the addend of the *_plus forms)
limb for limb; the carry-only forms are exact integers; tolerances are zero."""
import ctypes as C
import functools
import random

import numpy as np

from oracle.py import fields

MASK = (1 << 29) - 1
RR = 1 << 261
MODS = {0: fields.R, 1: fields.P}
FIELD_NAMES = {0: "Fr", 1: "Fq"}
SLOTS, OUT_LIMBS = 8, 18


def limbs(v):
    return [(v >> (29 * i)) & MASK for i in range(9)]


def value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


# ---- the operand tables the older tests were written around (moved here, unchanged) ------------------------------------------

def samples(N, rnd, bound_mult=2):
    """values below bound_mult * N: 0, 1, N - 1, N, N + 1, the top of the bound and one below, 2^253 - 1, every limb below the
    top saturated, and 40 seeded random ones (tests/test_emu_field29.py)"""
    top = bound_mult * N - 1
    vals = [0, 1, N - 1, N, N + 1, top, top - 1, (1 << 253) - 1, sum(MASK << (29 * i) for i in range(8)) % (bound_mult * N)]
    vals += [rnd.randrange(bound_mult * N) for _ in range(40)]
    return vals


def operand_sets(rng, n_mod, kind):
    """limbs of one Fe operand: normalized < 2N, or lazy (limbs < 2^30, e.g. 8N - x limb-wise) (tests/test_mont_asm.py)"""
    if kind == "norm":
        return limbs(rng.randrange(0, 2 * n_mod))
    if kind == "max":
        return limbs(2 * n_mod - 1)
    if kind == "allones":
        return [MASK] * 8 + [limbs(2 * n_mod - 1)[8]]
    if kind == "zero":
        return [0] * 9
    if kind == "lazy":  # 8N - x limb-wise with borrowed 2^29s (fe_neg_lazy): limbs in (0, 2^30), value <= 8N
        x, n8 = limbs(rng.randrange(0, 2 * n_mod)), limbs(8 * n_mod)
        return [n8[j] + ((1 << 29) if j < 8 else 0) - (1 if j > 0 else 0) - x[j] for j in range(9)]
    raise AssertionError(kind)


def worst_lazy31(n_mod):
    """the laziest operand the radix-4 NTT hands fe_mul (field.hip.h's contract; ntt.hip k_ntt_block4): eight limbs at 2^31 - 1 and a
    top limb that takes the value to just under 42 N"""
    low = [(1 << 31) - 1] * 8
    top = (42 * n_mod - 1 - value(low + [0])) >> 232
    l = low + [top]
    assert 41 * n_mod < value(l) < 42 * n_mod and top < (1 << 31)
    return l


# ---- operand classes ---------------------------------------------------------------------------------------------------------
# name -> (limbs(N, rng), value bound in multiples of N (value <= bound N), limb width in bits)

def lazy_neg(k, x, N):
    """k N - x limb-wise, every limb below the top inflated by the 2^29 it borrows from the next (fe_neg_lazy / fe_neg_lazy4);
    written from the definition, not from the NEG4 / NEG8 constants of field.hip.h"""
    kn = limbs(k * N)
    return [kn[j] + ((1 << 29) if j < 8 else 0) - (1 if j > 0 else 0) - x[j] for j in range(9)]


def _sat(k, N):
    """just below k N with every limb below the top saturated"""
    return limbs(((((k * N - 1) >> 232) - 1) << 232) | ((1 << 232) - 1))


def _sat30(N):
    low = [(1 << 30) - 1] * 8
    return low + [(8 * N - 1 - value(low + [0])) >> 232]


def _lazy31_rand(N, rng):
    return [rng.randrange(1 << 31) for _ in range(8)] + [rng.randrange(worst_lazy31(N)[8] + 1)]


CLASSES = {
    "zero": (lambda N, rng: limbs(0), 1, 29),
    "one": (lambda N, rng: limbs(1), 1, 29),
    "N-1": (lambda N, rng: limbs(N - 1), 1, 29),
    "N": (lambda N, rng: limbs(N), 1, 29),
    "N+1": (lambda N, rng: limbs(N + 1), 2, 29),
    "low8sat": (lambda N, rng: [MASK] * 8 + [0], 1, 29),
    "2^253-1": (lambda N, rng: limbs((1 << 253) - 1), 1, 29),
    "2^256-1": (lambda N, rng: limbs((1 << 256) - 1), 6, 29),
    "2^256-2": (lambda N, rng: limbs((1 << 256) - 2), 6, 29),
    "rand256": (lambda N, rng: limbs(rng.randrange(1 << 256)), 6, 29),
    "lazy8_rand": (lambda N, rng: lazy_neg(8, limbs(rng.randrange(2 * N)), N), 8, 30),     # test_mont_asm's `lazy`
    "lazy8_of_0": (lambda N, rng: lazy_neg(8, limbs(0), N), 8, 30),                         # the constant itself: the largest limbs
    "lazy8_of_top": (lambda N, rng: lazy_neg(8, limbs(2 * N - 1), N), 8, 30),
    "lazy_sat30": (lambda N, rng: _sat30(N), 8, 30),                                        # every limb below the top at 2^30 - 1
    "lazy4_rand": (lambda N, rng: lazy_neg(4, limbs(rng.randrange(2 * N)), N), 4, 30),
    "lazy4_of_0": (lambda N, rng: lazy_neg(4, limbs(0), N), 4, 30),
    "lazy4_of_top": (lambda N, rng: lazy_neg(4, limbs(2 * N - 1), N), 4, 30),
    "dbl_top2": (lambda N, rng: [2 * x for x in limbs(2 * N - 1)], 4, 30),
    "dbl_sat2": (lambda N, rng: [2 * x for x in _sat(2, N)], 4, 30),
    "dbl_rand2": (lambda N, rng: [2 * x for x in limbs(rng.randrange(2 * N))], 4, 30),
    "lazy31_worst": (lambda N, rng: worst_lazy31(N), 42, 31),
    "lazy31_rand": (_lazy31_rand, 42, 31),
}
for _k in (2, 4, 6, 8, 10):
    CLASSES[f"top{_k}"] = (lambda N, rng, k=_k: limbs(k * N - 1), _k, 29)
    CLASSES[f"top{_k}-1"] = (lambda N, rng, k=_k: limbs(k * N - 2), _k, 29)
    CLASSES[f"sat{_k}"] = (lambda N, rng, k=_k: _sat(k, N), _k, 29)
    CLASSES[f"rand{_k}"] = (lambda N, rng, k=_k: limbs(rng.randrange(k * N)), _k, 29)

_LOW = ["zero", "one", "N-1", "N", "N+1", "low8sat", "2^253-1"]
N2 = _LOW + ["top2", "top2-1", "sat2", "rand2"]                  # almost reduced: what every routine hands on
W4 = ["top4", "sat4", "rand4"]
W6 = ["top6", "top6-1", "sat6", "rand6"]                         # f_mul_minus / f_mul_minus_y results
W8 = ["top8", "top8-1", "sat8", "rand8"]                         # "fe_mul tolerates operands up to 8N"
W10 = ["top10", "top10-1", "sat10", "rand10"]                    # f_add2_weak(P, X1), the d of f_sqr_sub
L8 = ["lazy8_rand", "lazy8_of_0", "lazy8_of_top", "lazy_sat30"]
L4 = ["lazy4_rand", "lazy4_of_0", "lazy4_of_top"]
DBL = ["dbl_top2", "dbl_sat2", "dbl_rand2"]
L31 = ["lazy31_worst", "lazy31_rand"]
ANY256 = _LOW + ["top2", "sat2", "2^256-1", "2^256-2", "rand256"]
NZ2 = ["one", "N-1", "N+1", "low8sat", "2^253-1", "top2", "sat2", "rand2"]   # fe_inv: a != 0

# fe_neg_lazy / fe_neg_lazy4 take a normalized a whose top limb is below that of 8N / 4N (sat8 / sat4 is the largest such value)
for _k in (4, 8):
    CLASSES[f"rand{_k}s"] = (lambda N, rng, k=_k: limbs(rng.randrange(((k * N) >> 232) << 232)), _k, 29)
S8 = ["sat8", "rand8s"]
S4 = ["sat4", "rand4s"]

for _fam in (S4, S8, N2, W4, W6, W8, W10, L8, L4, DBL, L31, ANY256, NZ2):
    assert all(c in CLASSES for c in _fam)


def is_extreme(cname):
    return "rand" not in cname


def fam_bound(fam):
    return max(CLASSES[c][1] for c in fam)


def fam_bits(fam):
    return max(CLASSES[c][2] for c in fam)


# ---- the reference -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _ninv(N):
    return pow(N, -1, RR)


def mont(total, N):
    """what every product routine returns for a sum of products `total`: exact, not just a residue"""
    m = (-total * _ninv(N)) % RR
    q, r = divmod(total + m * N, RR)
    assert r == 0
    return q


def _red2(v, N):
    return v - 2 * N if v >= 2 * N else v


def _inv_chain(a, N):
    """fe_inv's square-and-multiply over the bits of N - 2, most significant of 9 x 29 first, on exact Montgomery products"""
    r, e = RR % N, N - 2
    for bit in range(9 * 29 - 1, -1, -1):
        r = mont(r * r, N)
        if (e >> bit) & 1:
            r = mont(r * a, N)
    return r


class Op:
    """terms: the sum of products of a Montgomery form as ("mul", i, j) / ("sqr", i) over operand positions; plus: the position of
    the addend of a *_plus form; max_lazy: how many products may hold an operand with limbs >= 2^29; bound: result < bound N"""

    def __init__(self, name, num, arity, profiles, ref, fields=(0, 1), terms=None, plus=None, max_lazy=None, bound=None,
                 asm=None, extra=None, reps=4, n_random=48, out_fe=1, both_lazy=False):
        self.name, self.num, self.arity, self.profiles, self.ref, self.fields = name, num, arity, profiles, ref, fields
        self.terms, self.plus, self.max_lazy, self.bound, self.asm, self.extra = terms, plus, max_lazy, bound, asm, extra
        self.reps, self.n_random, self.out_fe, self.both_lazy = reps, n_random, out_fe, both_lazy
        assert all(len(p) == arity for p in profiles), name


def _product_total(op, v):
    t = 0
    for term in op.terms:
        t += v[term[1]] * v[term[2]] if term[0] == "mul" else v[term[1]] ** 2
    return t


def _product_contract(op, ls, N):
    """the contract field.hip.h documents for the product forms, on the limbs of one case"""
    v = [value(l) for l in ls]
    lazy_products = 0
    for term in op.terms:
        if term[0] == "sqr":
            assert max(ls[term[1]]) <= MASK, "the squared operand is normalized"
            continue
        x, y = ls[term[1]], ls[term[2]]
        wide = [l for l in (x, y) if max(l) > MASK]
        if wide:
            lazy_products += 1
        if any(max(l) >= 1 << 30 for l in (x, y)):
            # fe_mul alone: ONE operand with limbs < 2^31 and a value up to 42 N against a normalized partner < 2N
            assert op.name == "fe_mul" and len(wide) == 1 and max(wide[0]) < 1 << 31 and value(wide[0]) <= 42 * N
            other = y if wide[0] is x else x
            assert max(other) <= MASK and value(other) < 2 * N
        elif len(wide) == 2:
            assert op.both_lazy, "at most one lazy operand per product"   # fe_mul: "operands: limbs < 2^30"
    assert lazy_products <= op.max_lazy, "too many products with a lazy operand for one 64-bit column"
    assert _product_total(op, v) < 169 * N * N
    if op.plus is not None:
        assert max(ls[op.plus]) < 1 << 30 and v[op.plus] <= 4 * N


def _product_ref(op):
    def ref(ls, N):
        v = [value(l) for l in ls]
        r = mont(_product_total(op, v), N)
        assert r < 2 * N                      # the routines' own claim, from the contract alone
        if op.plus is not None:
            r += v[op.plus]
        return limbs(r)
    return ref


def _product_op(name, num, arity, profiles, terms, plus=None, max_lazy=1, asm=None, **kw):
    op = Op(name, num, arity, profiles, None, terms=terms, plus=plus, max_lazy=max_lazy, bound=6 if plus is not None else 2, asm=asm, **kw)
    op.ref = _product_ref(op)
    op.contract = lambda ls, N, op=op: _product_contract(op, ls, N)
    return op


def _norm_contract(bounds):
    """every operand normalized and below its bound (in multiples of N; None: any 256-bit value)"""
    def contract(ls, N):
        for l, b in zip(ls, bounds):
            assert max(l) <= MASK and value(l) < (b * N if b else 1 << 256)
    return contract


def _simple_op(name, num, profiles, bounds, ref, **kw):
    op = Op(name, num, len(bounds), profiles, lambda ls, N: ref([value(l) for l in ls], ls, N), **kw)
    op.contract = _norm_contract(bounds)
    return op


def _flag(t, second=None):
    return [1 if t else 0, 0 if second is None else (1 if second else 0)] + [0] * 7


def _eq_extra(N, rng):
    out = []
    for a in (0, 1, 5, N - 1, rng.randrange(N)):
        for b in (a, a + N):
            out.append(([limbs(a), limbs(b)], ("eq_pair", "eq_pair")))
            out.append(([limbs(b), limbs(a)], ("eq_pair", "eq_pair")))
            out.append(([limbs(b), limbs(b)], ("eq_pair", "eq_pair")))
    return out


def _weak_diff_extra(N, rng):
    """d = a - b + 4N for a, b in [0, 2N): the three zeros 3N, 4N, 5N, their neighbours, and values that share limb 0 (the early
    exit) or all limbs but one with a zero"""
    out = []
    for k in (3, 4, 5):
        z = limbs(k * N)
        out.append(([z], (f"{k}N",)))
        for d in (k * N - 1, k * N + 1):
            out.append(([limbs(d)], (f"{k}N+-1",)))
        for j in range(1, 9):
            l = list(z)
            l[j] ^= 1 << rng.randrange(29 if j < 8 else 20)
            if 2 * N < value(l) < 6 * N:
                out.append(([l], (f"{k}N_flip_limb{j}",)))
    for _ in range(64):
        a, b = rng.randrange(2 * N), rng.randrange(2 * N)
        out.append(([limbs(a - b + 4 * N)], ("diff_rand",)))
        out.append(([limbs(a - (a % N) + 4 * N)], ("diff_zero",)))   # b = a mod N
    out.append(([limbs(2 * N + 1)], ("diff_min",)))
    out.append(([limbs(6 * N - 1)], ("diff_max",)))
    return out


def _weak_diff_contract(ls, N):
    assert max(ls[0]) <= MASK and 2 * N < value(ls[0]) < 6 * N


def _build_ops():
    ops = []
    add = ops.append
    # -- the nine asm statements, each reached directly --
    add(_product_op("fe_mul", 2, 2, [(N2, N2), (W6, W6), (W8, W8), (W10, W10), (L8, N2), (N2, L8), (L8, W10), (W10, L8), (L8, L8),
                                      (L31, N2), (N2, L31), (DBL, W8)], [("mul", 0, 1)], asm="MUL", both_lazy=True))
    add(_product_op("fe_sqr", 3, 1, [(N2,), (W6,), (W8,), (W10,)], [("sqr", 0)], asm="SQR", max_lazy=0, reps=1, n_random=200))
    add(_product_op("fe_sqr_add", 20, 3, [(N2, N2, N2), (W8, L8, W8), (W6, L4, W10), (W10, L8, N2), (N2, DBL, W8)],
                    [("sqr", 0), ("mul", 1, 2)], asm="SQR_ADD"))
    add(_product_op("fe_mul_add", 21, 4, [(N2, N2, N2, N2), (W6, W6, L8, W6), (L8, N2, N2, L8), (N2, L8, L4, W10), (W8, W8, W8, W8),
                                          (DBL, W8, L8, W8)], [("mul", 0, 1), ("mul", 2, 3)], asm="MUL_ADD", max_lazy=2))
    add(_product_op("fe_mul_plus", 22, 3, [(N2, N2, L4), (N2, N2, N2), (L4, N2, L4), (L8, N2, L4), (N2, L8, L4), (W6, W6, L4)],
                    [("mul", 0, 1)], plus=2, asm="MUL_PLUS"))
    add(_product_op("fe_mul_add_plus", 23, 5, [(N2, N2, L8, N2, L4), (L4, N2, N2, N2, L4), (L4, N2, L4, N2, L4), (N2, N2, N2, N2, N2),
                                               (W6, N2, L8, N2, L4)], [("mul", 0, 1), ("mul", 2, 3)], plus=4, asm="MUL_ADD_PLUS", max_lazy=2))
    # f_sqr_sub's imaginary part holds three lazy operands: 3 x 9 x 2^59 + 9 x 2^58 (reduction) + carry < 2^64
    add(_product_op("fe_mul_add3", 24, 6, [(DBL, W6, L4, W10, L4, W10), (N2,) * 6, (L8, N2, N2, L8, L8, N2)],
                    [("mul", 0, 1), ("mul", 2, 3), ("mul", 4, 5)], asm="MUL_ADD3", max_lazy=3))
    add(_product_op("fe_mul_add4", 25, 8, [(W6, W6, L8, W6, L8, N2, N2, N2), (W6, W6, W6, W6, L8, N2, L8, N2), (N2,) * 8,
                                           (N2, L8, N2, N2, N2, N2, L4, N2)], [("mul", 0, 1), ("mul", 2, 3), ("mul", 4, 5), ("mul", 6, 7)],
                    asm="MUL_ADD4", max_lazy=2, reps=3))
    # as f_sqr_sub uses it: two products with a lazy operand beside the squaring (9 x 2^58 (1 + 4 + 1 + 1) + carry < 2^64)
    add(_product_op("fe_sqr_add3", 26, 7, [(W6, L8, W6, L4, W10, N2, W10), (N2,) * 7, (W8, N2, N2, L8, N2, N2, L8)],
                    [("sqr", 0), ("mul", 1, 2), ("mul", 3, 4), ("mul", 5, 6)], asm="SQR_ADD3", max_lazy=2, reps=3))
    # -- what feeds them --
    add(_simple_op("fe_add", 0, [(N2, N2)], (2, 2), lambda v, ls, N: limbs(_red2(v[0] + v[1], N)), bound=2))
    add(_simple_op("fe_sub", 1, [(N2, N2)], (2, 2), lambda v, ls, N: limbs(_red2(v[0] - v[1] + 2 * N, N)), bound=2))
    add(_simple_op("fe_neg", 5, [(N2,)], (2,), lambda v, ls, N: limbs(_red2(2 * N - v[0], N)), bound=2, reps=1, n_random=200))
    add(_simple_op("fe_dbl", 27, [(N2,)], (2,), lambda v, ls, N: limbs(_red2(2 * v[0], N)), bound=2, reps=1, n_random=200))
    add(_simple_op("fe_add_lazy", 28, [(N2, N2), (W10, W10)], (10, 10), lambda v, ls, N: [x + y for x, y in zip(ls[0], ls[1])]))
    add(_simple_op("fe_neg_lazy", 29, [(N2,), (W6,), (S8,)], (8,), lambda v, ls, N: lazy_neg(8, ls[0], N), reps=1, n_random=200))
    add(_simple_op("fe_neg_lazy4", 30, [(N2,), (S4,)], (4,), lambda v, ls, N: lazy_neg(4, ls[0], N), reps=1, n_random=200))
    for k in (8, 4):    # the bound is on the top limb (field.hip.h): a < floor(k N / 2^232) 2^232
        ops[-1 if k == 4 else -2].contract = lambda ls, N, k=k: _assert(max(ls[0]) <= MASK and ls[0][8] < limbs(k * N)[8])
    add(_simple_op("fe_dbl_lazy", 31, [(N2,), (W8,)], (8,), lambda v, ls, N: [2 * x for x in ls[0]], reps=1, n_random=200))
    add(_simple_op("fe_sub_weak", 12, [(N2, N2), (W6, N2), (W10, W4)], (10, 4), lambda v, ls, N: limbs(v[0] - v[1] + 4 * N)))
    add(_simple_op("fe_add2_weak", 13, [(N2, N2), (W6, N2)], (6, 2), lambda v, ls, N: limbs(v[0] + 2 * v[1])))
    add(_simple_op("fe_add3_weak", 32, [(N2, N2, N2), (W6, W6, W6)], (6, 6, 6), lambda v, ls, N: limbs(v[0] + v[1] + v[2])))
    wd = Op("fe_weak_diff_is_zero", 33, 1, [], lambda ls, N: _flag((value(ls[0]) - 4 * N) % N == 0), extra=_weak_diff_extra)
    wd.contract = _weak_diff_contract
    add(wd)
    # -- entries and exits --
    add(_simple_op("fe_canon", 34, [(N2,)], (2,), lambda v, ls, N: limbs(v[0] % N), bound=1, reps=1, n_random=200))
    add(_simple_op("fe_lt_modulus", 35, [(ANY256,)], (None,), lambda v, ls, N: _flag(v[0] < N), reps=1, n_random=200))
    add(_simple_op("fe_from_mont", 4, [(N2,)], (2,), lambda v, ls, N: limbs(mont(v[0], N) % N), bound=1, reps=1, n_random=200))
    add(_simple_op("fe_to_mont", 36, [(ANY256,)], (None,), lambda v, ls, N: limbs(mont(v[0] * (RR * RR % N), N)), bound=2, reps=1, n_random=200))
    add(_simple_op("fe_words_roundtrip", 7, [(ANY256,)], (None,), lambda v, ls, N: limbs(v[0]), reps=1, n_random=200))
    add(_simple_op("fe_eq_is_zero", 8, [(N2, N2)], (2, 2), lambda v, ls, N: _flag((v[0] - v[1]) % N == 0, v[0] % N == 0), extra=_eq_extra))
    add(_simple_op("fe_inv", 6, [(NZ2,)], (2,), lambda v, ls, N: limbs(_inv_chain(v[0], N)), bound=2, reps=1, n_random=24))
    ops[-1].contract = lambda ls, N: (_norm_contract((2,))(ls, N), _assert(value(ls[0]) % N != 0))
    # -- the Fq2 layer of ec.hip.h (Fq only; an Fq2 operand is two positions) --
    n8 = lambda x, N: 8 * N - x
    n4 = lambda x, N: 4 * N - x

    def fq2(name, num, arity, profiles, bounds, comps, negated, minus=None, **kw):
        """comps(v, N) -> the two sums of products; minus: positions of the x whose 4N - x rides in the high columns"""
        def ref(ls, N):
            v = [value(l) for l in ls]
            out = []
            for k, tot in enumerate(comps(v, N)):
                assert tot < 169 * N * N
                r = mont(tot, N)
                assert r < 2 * N
                out += limbs(r + (4 * N - v[minus[k]] if minus else 0))
            return out
        op = Op(name, num, arity, profiles, ref, fields=(1,), out_fe=2, bound=6 if minus else 2, **kw)

        def contract(ls, N):
            _norm_contract(bounds)(ls, N)
            for pos, k in negated:
                assert ls[pos][8] < limbs(k * N)[8]      # fe_neg_lazy / fe_neg_lazy4: the bound is on the top limb
            for tot in comps([value(l) for l in ls], N):
                assert tot < 169 * N * N
        op.contract = contract
        return op

    add(fq2("f_mul", 64, 4, [(N2,) * 4, (W6, W6, N2, N2), (N2, N2, W6, W6), (W6,) * 4], (8, 8, 8, 8),
            lambda v, N: (v[0] * v[2] + n8(v[1], N) * v[3], v[0] * v[3] + v[1] * v[2]), [(1, 8)]))
    add(fq2("f_sqr", 65, 2, [(N2, N2), (W6, W6), (W8, S8)], (8, 8),
            lambda v, N: (v[0] ** 2 + n8(v[1], N) * v[1], 2 * v[0] * v[1]), [(1, 8)]))
    add(fq2("f_mul_sub", 66, 8, [(N2,) * 8, (W6,) * 4 + (N2,) * 4], (6, 6, 6, 6, 2, 2, 2, 2),
            lambda v, N: (v[0] * v[2] + n8(v[1], N) * v[3] + n8(v[4], N) * v[6] + v[5] * v[7],
                          v[0] * v[3] + v[1] * v[2] + n8(v[4], N) * v[7] + n8(v[5], N) * v[6]), [(1, 8), (4, 8), (5, 8)], reps=3))
    add(fq2("f_sqr_sub", 67, 6, [(N2,) * 6, (W6, W6, N2, N2, W10, W10)], (6, 6, 2, 2, 10, 10),
            lambda v, N: (v[0] ** 2 + n8(v[1], N) * v[1] + n4(v[2], N) * v[4] + v[3] * v[5],
                          2 * v[0] * v[1] + n4(v[2], N) * v[5] + n4(v[3], N) * v[4]), [(1, 8), (2, 4), (3, 4)]))
    add(fq2("f_mul_minus", 68, 6, [(N2,) * 6], (2,) * 6,
            lambda v, N: (v[0] * v[2] + n8(v[1], N) * v[3], v[0] * v[3] + v[1] * v[2]), [(1, 8), (4, 4), (5, 4)], minus=(4, 5)))
    add(fq2("f_mul_minus_y_pos", 69, 6, [(N2,) * 6], (2,) * 6,
            lambda v, N: (v[0] * v[2] + n8(v[1], N) * v[3], v[0] * v[3] + v[1] * v[2]), [(0, 4), (1, 4), (1, 8), (4, 4), (5, 4)], minus=(4, 5)))
    add(fq2("f_mul_minus_y_neg", 70, 6, [(N2,) * 6], (2,) * 6,
            lambda v, N: (n4(v[0], N) * v[2] + v[1] * v[3], n4(v[0], N) * v[3] + n4(v[1], N) * v[2]), [(0, 4), (1, 4), (1, 8), (4, 4), (5, 4)], minus=(4, 5)))
    return ops


def _assert(c):
    assert c


OPS = {op.name: op for op in _build_ops()}
assert len({op.num for op in OPS.values()}) == len(OPS)
PARAMS = [(name, f) for name, op in OPS.items() for f in op.fields]


class Case:
    __slots__ = ("limbs", "classes")

    def __init__(self, ls, classes):
        self.limbs, self.classes = ls, tuple(classes)


@functools.lru_cache(None)
def table(name, field):
    """the cases of one (op, field), in a fixed order (seeded)"""
    op, N = OPS[name], MODS[field]
    rng = random.Random(f"field_raw/{name}/{field}")
    cases, turn = [], 0

    def emit(ls, classes):
        op.contract(ls, N)            # a condition on the generator, not a filter: a violation fails the table
        cases.append(Case(ls, classes))

    for prof in op.profiles:
        # the documented sum bound holds for the worst members of the families together
        if op.terms:
            b = [fam_bound(f) for f in prof]
            assert sum(b[t[1]] * b[t[2]] if t[0] == "mul" else b[t[1]] ** 2 for t in op.terms) < 169, (name, prof)
        for pos, fam in enumerate(prof):
            for cname in fam:
                for _ in range(op.reps if is_extreme(cname) else 1):
                    turn += 1
                    classes = [cname if q == pos else prof[q][(turn + 3 * q) % len(prof[q])] for q in range(op.arity)]
                    emit([CLASSES[c][0](N, rng) for c in classes], classes)
        for _ in range(op.n_random):
            classes = [rng.choice(f) for f in prof]
            emit([CLASSES[c][0](N, rng) for c in classes], classes)
    if op.extra:
        for ls, classes in op.extra(N, rng):
            emit(ls, classes)
    return tuple(cases)


def required_coverage(name):
    """(profile index, position, class) for every named extreme class a profile admits in a position"""
    return {(k, pos, c) for k, prof in enumerate(OPS[name].profiles) for pos, fam in enumerate(prof) for c in fam if is_extreme(c)}


def expected(name, field, case):
    exp = list(OPS[name].ref(case.limbs, MODS[field]))
    return exp + [0] * (OUT_LIMBS - len(exp))


def check(name, field, cases, got):
    """got: n x 18 limbs as the routine returned them.  Zero tolerance."""
    op, N = OPS[name], MODS[field]
    assert len(got) == len(cases)
    for k, (case, g) in enumerate(zip(cases, got)):
        g = [int(x) for x in g]
        where = f"{name} {FIELD_NAMES[field]} case {k} classes {case.classes}"
        exp = expected(name, field, case)
        if op.bound is not None:          # a field value comes back: normalized limbs, below the bound the routine documents
            for j in range(op.out_fe):
                part = g[9 * j:9 * j + 9]
                assert all(x <= MASK for x in part), f"{where}: limbs not normalized {part}"
                assert value(part) < op.bound * N, f"{where}: value not below {op.bound} N"
        if op.name in ("fe_add", "fe_sub", "fe_neg", "fe_dbl"):
            v = [value(l) for l in case.limbs]
            want = {"fe_add": lambda: v[0] + v[1], "fe_sub": lambda: v[0] - v[1], "fe_neg": lambda: -v[0], "fe_dbl": lambda: 2 * v[0]}[op.name]()
            assert (value(g[:9]) - want) % N == 0, f"{where}: not congruent"
        if op.plus is not None:
            assert value(g[:9]) < 2 * N + value(case.limbs[op.plus]), f"{where}: above 2N + the addend"
        if op.name == "fe_inv":
            x = value(case.limbs[0]) * pow(RR, -1, N) % N
            assert value(g[:9]) % N == pow(x, -1, N) * RR % N, f"{where}: not the inverse"
        if g != exp:
            j = next(i for i in range(OUT_LIMBS) if g[i] != exp[i])
            raise AssertionError(f"{where}: limb {j} is {g[j]:#x}, expected {exp[j]:#x}\n operands {[[hex(x) for x in l] for l in case.limbs]}\n"
                                 f" got      {[hex(x) for x in g]}\n expected {[hex(x) for x in exp]}")


def pack(cases):
    arr = np.zeros((len(cases), SLOTS, 9), dtype=np.uint32)
    for k, c in enumerate(cases):
        arr[k, :len(c.limbs)] = np.array(c.limbs, dtype=np.uint64).astype(np.uint32)
    return arr


def run(ctx, name, field):
    """one upload, ONE call of og_hook_fe_raw_d (one launch), one download, compared with the reference.  ctx: a context of a
    hooks build -- libowshen_gpu_hooks.so on the GPU or the CPU interpreter's library"""
    cases = table(name, field)
    fn = ctx._lib.og_hook_fe_raw_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    d_in = ctx.to_device(pack(cases))
    d_out = ctx.empty(len(cases) * OUT_LIMBS * 4)
    ctx._pre()
    ctx._check(fn(ctx._h, field, OPS[name].num, ctx.ptr(d_in), len(cases), ctx.ptr(d_out)))
    got = np.asarray(ctx.to_host(d_out)).view(np.uint32).reshape(len(cases), OUT_LIMBS)
    check(name, field, cases, got.tolist())
    return len(cases)
