"""The wave-wide G1 group law (owshen_amd/csrc/ec_w9.hip.h) walked alone at the edge of its bounds table -- TEST INFRASTRUCTURE ONLY.

og_hook_w9_ec_chain_d (hooks build) walks one chain per WAVE with w9_xyzz_dbl / w9_xyzz_add and nothing in between, from an
accumulator handed in as raw spread limbs and back out as the word of all 64 lanes.  A chain has the shape of k_assemble_g1_muls_w9:
the table build (2 P by doubling, then + P thirteen times), the first digit (acc = table[d]), then 31 windows of four doublings and
one addition of a table entry -- 14 + 1 + 31 x 5 = 170 steps, a walked scalar below 2^127 with no zero nibble, so no equal or
opposite operands meet (the law has no branch for them).

Starting points: X = x + j N for every admissible j (0 .. 9, below 9.3 N), Y = y + j N for j 0 .. 5 (below 5.7 N), ZZ / ZZZ plus N
where that stays below 1.2 N, the scaling picked among 400 draws so that one coordinate lies just under its bound.  The operands of
the additions are the model's own table entries, in every other chain re-represented the same way (another admissible j per
coordinate).  Limbs: normalized, or with carries pushed down as far as 2^30 - 1 allows -- past the 2^29 + 32 a product leaves (a
point's coordinates cannot be given limbs in [2^29, 2^29 + 32): that needs a normalized limb below 32), inside what the products
and U = 2 Y take (limbs below 2^31).

Every chain is also cut after 1, 2, 5, 20 and 100 steps and run once more with the kernel's exit step last.  The reference is the
law restated on Python integers limb by limb (w9_raw_cases.lane_mul, itself pinned to the closed form of the strict product), with
every hard precondition asserted on the way: a b < 169 N^2, limbs below 2^31 into a product and below 2^32 into a carry, a
subtrahend below (K - 2) N with limbs below 2^30 - 2.  Checked at every cut, zero tolerance: the limbs and so the VALUES of the four
coordinates, lanes 9 .. 63 zero, X < 9.3 N, Y < 5.7 N, ZZ, ZZZ < 1.2 N (below 2 N and normalized after the exit), and the affine
point against oracle/py/curve for the same scalar."""
import ctypes as C
import functools
import random

import numpy as np

from oracle.py import fields
from oracle.py.curve import G1, G1_GEN
from tests.w9_raw_cases import MASK, M32, RR, carry_model, kn_limbs, lane_mul, limbs, pushed, strict_value, value

P = fields.P
F = G1.F
N_CHAINS, N_STEPS, REC = 40, 170, 1 + 4 * 9
CUTS = (1, 2, 5, 20, 100, N_STEPS)
EC_CEIL = (1 << 30) - 1
BOUNDS = (930, 570, 120, 120)            # X, Y, ZZ, ZZZ in hundredths of N
DBL, ADD, SET, EXIT, NOP = 0, 1, 2, 3, 4
ONE = limbs(RR % P)


class Maxima(dict):
    def see(self, key, v):
        self[key] = max(self.get(key, 0), v * 1000 // P)


SEEN = Maxima()


def _mul(a, b):
    assert max(a) < 1 << 31 and max(b) < 1 << 31, "a limb above 2^31 goes into a product"
    assert value(a) * value(b) < 169 * P * P, "a b above 169 N^2 goes into a strict product"
    r = lane_mul(a, b, P, False)
    assert value(r) == strict_value(value(a), value(b), P)
    return r


def _carry(x):
    assert max(x) <= M32, "a limb above 2^32 goes into a carry"
    return carry_model(x)


def _sub(a, b, K):
    assert value(b) < (K - 2) * P and max(b) <= (1 << 30) - 3, f"a subtrahend outside what w9_kn_limb<{K}> admits"
    raw = [x + c - y for x, c, y in zip(a, kn_limbs(P, K), b)]
    assert min(raw) >= 0
    return raw


def w9_dbl(p):
    X, Y, ZZ, ZZZ = p
    U = [2 * y for y in Y]
    V = _mul(U, U)
    W = _mul(U, V)
    S = _mul(X, V)
    M = [3 * m for m in _mul(X, X)]
    X3 = _carry(_sub(_mul(M, M), _carry([2 * s for s in S]), 8))
    D = _carry(_sub(S, X3, 16))
    Y3 = _carry(_sub(_mul(M, D), _mul(W, Y), 4))
    for key, v in (("U", U), ("M", M), ("D", D)):
        SEEN.see(key, value(v))
    return (X3, Y3, _mul(V, ZZ), _mul(W, ZZZ))


def w9_add(a, b):
    U1, S1 = _mul(b[2], a[0]), _mul(b[3], a[1])
    Pd, R = _carry(_sub(_mul(a[2], b[0]), U1, 4)), _carry(_sub(_mul(a[3], b[1]), S1, 4))
    PP = _mul(Pd, Pd)
    PPP, Q = _mul(PP, Pd), _mul(PP, U1)
    X3 = _carry(_sub(_mul(R, R), _carry([x + 2 * q for x, q in zip(PPP, Q)]), 8))
    D = _carry(_sub(Q, X3, 16))
    Y3 = _carry(_sub(_mul(R, D), _mul(PPP, S1), 4))
    for key, v in (("P,R", Pd), ("P,R", R), ("D", D)):
        SEEN.see(key, value(v))
    return (X3, Y3, _mul(PP, _mul(a[2], b[2])), _mul(PPP, _mul(a[3], b[3])))


def w9_exit(p):
    return tuple(limbs(value(_mul(ONE, c))) for c in p)


def _within(vals):
    return all(v * 100 < b * P for v, b in zip(vals, BOUNDS))


def _represent(res, js, slack, rnd):
    """four Montgomery residues -> limbs of residue + j N, normalized or pushed down"""
    vals = [r + j * P for r, j in zip(res, js)]
    assert _within(vals)
    return tuple(pushed(v, EC_CEIL, rnd if slack == 2 else None) if slack else limbs(v) for v in vals)


def _largest_js(res, rnd, top=False):
    """an admissible j per coordinate: random, or (top) the largest"""
    js = []
    for r, b, most in zip(res, BOUNDS, (9, 5, 1, 1)):
        ok = [j for j in range(most + 1) if (r + j * P) * 100 < b * P]
        js.append(ok[-1] if top else rnd.choice(ok))
    return js


def _start(pt, jx, jy, aim, rnd):
    """the XYZZ form (x l^2, y l^3, l^2, l^3) of pt under the scaling, among 400 draws, that admits X + jx N and Y + jy N and brings
    the aimed coordinate closest under its bound (aim 0 / 1: X / Y largest; 2 / 3: ZZ / ZZZ smallest, so that + N is admissible)"""
    best, key = None, None
    for _ in range(400):
        lam = rnd.randrange(1, P)
        l2 = F.sqr(lam)
        l3 = F.mul(l2, lam)
        res = [F.mul(pt[0], l2) * RR % P, F.mul(pt[1], l3) * RR % P, l2 * RR % P, l3 * RR % P]
        if not _within([res[0] + jx * P, res[1] + jy * P, res[2], res[3]]):
            continue
        k = res[aim] if aim < 2 else -res[aim]
        if key is None or k > key:
            best, key = res, k
    assert best is not None
    js = [jx, jy] + [1 if (r + P) * 100 < 120 * P else 0 for r in best[2:]]
    return best, js


# (jx, jy) of the forty chains: every admissible j of X and of Y, and more than a quarter each at X >= 8 N and at Y >= 4 N
_JX = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9] + [8, 9] * 5 + [0, 9, 3, 8, 5, 9, 1, 8, 7, 9] + [2, 4, 6, 0, 9, 8, 1, 3, 5, 7]
_JY = [0, 1, 2, 3, 4, 5] * 2 + [4, 5] * 8 + [0, 5, 1, 4, 2, 5, 3, 4, 5, 0, 4, 1]


class Chain:
    pass


@functools.lru_cache(None)
def build():
    """-> the forty chains (acc limbs, step records, the model's accumulator and the scalar after every step), walked ONCE"""
    assert len(_JX) == len(_JY) == N_CHAINS
    chains = []
    for c in range(N_CHAINS):
        rnd = random.Random(f"w9_ec_chain/{c}")
        ch = Chain()
        ch.c, ch.jx, ch.jy, ch.slack, ch.boost = c, _JX[c], _JY[c], c % 3, c % 2 == 1
        s = rnd.randrange(1, fields.R)
        pt = G1.mul(G1_GEN, s)
        res, js = _start(pt, ch.jx, ch.jy, (c // 2) % 4, rnd)
        base = _represent(res, js, ch.slack, rnd)
        ch.acc = base
        digits = [15] * 32 if c == 7 else [rnd.randrange(1, 16) for _ in range(32)]      # d_31 first
        tab, recs, after, scal = {1: base}, [], [], []
        acc, m = base, 1

        def step(kind, operand=None, dm=None):
            nonlocal acc, m
            recs.append([kind] + ([x for co in operand for x in co] if operand is not None else [0] * 36))
            if kind == DBL:
                acc, m = w9_dbl(acc), 2 * m
            elif kind == ADD:
                acc, m = w9_add(acc, operand), m + dm
            else:
                acc, m = operand, dm
            for key, co in zip(("X", "Y", "ZZ", "ZZZ"), acc):
                SEEN.see(key, value(co))
            after.append(acc)
            scal.append(m * s % fields.R)

        for d in range(2, 16):
            step(DBL) if d == 2 else step(ADD, base, 1)
            tab[d] = acc

        def entry(d):
            if not ch.boost:
                return tab[d]
            res = [value(co) % P for co in tab[d]]
            return _represent(res, _largest_js(res, rnd, top=rnd.randrange(4) == 0), rnd.randrange(3), rnd)

        step(SET, entry(digits[0]), digits[0])
        for d in digits[1:]:
            for _ in range(4):
                step(DBL)
            step(ADD, entry(d), d)
        assert len(recs) == N_STEPS and m < 1 << 128
        ch.recs, ch.after, ch.scal = recs, after, scal
        ch.exit = w9_exit(acc)
        chains.append(ch)
    return tuple(chains)


def coverage(chains):
    """what the starting points reach, asserted by run() and by the CPU test over all forty chains"""
    n = len(chains)
    xs, ys = [value(ch.acc[0]) for ch in chains], [value(ch.acc[1]) for ch in chains]
    return {"n": n, "x_ge_8N": sum(x >= 8 * P for x in xs), "y_ge_4N": sum(y >= 4 * P for y in ys),
            "jx": {x // P for x in xs}, "jy": {y // P for y in ys},
            "zz_ge_N": sum(value(ch.acc[2]) >= P for ch in chains), "zzz_ge_N": sum(value(ch.acc[3]) >= P for ch in chains),
            "x_max": max(xs) * 1000 // P, "y_max": max(ys) * 1000 // P,
            "pushed": sum(max(max(co) for co in ch.acc) > MASK for ch in chains)}


GROUPS = tuple(tuple(range(g, N_CHAINS, 8)) for g in range(8))     # five chains each, every group with small and large j


def run(ctx, which, cuts=CUTS):
    """one launch of og_hook_w9_ec_chain_d: a wave per (chain of `which`, cut) and per chain one more with the exit step; -> waves
    checked.  The coverage conditions are asserted over all forty chains, whichever of them this launch walks."""
    cov = coverage(build())
    assert cov["n"] == N_CHAINS and 4 * cov["x_ge_8N"] >= cov["n"] and 4 * cov["y_ge_4N"] >= cov["n"], cov
    assert cov["jx"] == set(range(10)) and cov["jy"] == set(range(6)) and cov["zz_ge_N"] and cov["zzz_ge_N"] and cov["pushed"], cov
    chains = [build()[c] for c in which]
    n_steps = N_STEPS + 1
    pad = [NOP] + [0] * 36
    accs, steps, expect = [], [], []
    for ch in chains:
        for cut in cuts + ("exit",):
            k = N_STEPS if cut == "exit" else cut
            accs.append([x for co in ch.acc for x in co])
            steps.append(ch.recs[:k] + ([[EXIT] + [0] * 36] if cut == "exit" else []) + [pad] * (n_steps - k - (cut == "exit")))
            expect.append((ch, cut, ch.exit if cut == "exit" else ch.after[k - 1], ch.scal[k - 1]))
    n = len(expect)
    accs = np.array(accs, dtype=np.uint64).astype(np.uint32)
    steps = np.array(steps, dtype=np.uint64).astype(np.uint32)
    assert accs.shape == (n, 36) and steps.shape == (n, n_steps, REC)
    fn = ctx._lib.og_hook_w9_ec_chain_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    d_acc, d_steps = ctx.to_device(accs), ctx.to_device(steps)
    d_out = ctx.empty(n * 4 * 64 * 4)
    ctx._pre()
    ctx._check(fn(ctx._h, ctx.ptr(d_acc), ctx.ptr(d_steps), n, n_steps, ctx.ptr(d_out)))
    out = np.asarray(ctx.to_host(d_out)).view(np.uint32).reshape(n, 4, 64)
    for k, (ch, cut, want, scalar) in enumerate(expect):
        where = f"chain {ch.c} (jx {ch.jx}, jy {ch.jy}, slack {ch.slack}, boost {ch.boost}) cut {cut}"
        assert not out[k, :, 9:].any(), f"{where}: a lane outside the nine limbs is not zero"
        got = [[int(x) for x in out[k, co, :9]] for co in range(4)]
        vals = [value(g) for g in got]
        for name, g, w in zip(("X", "Y", "ZZ", "ZZZ"), got, want):
            assert value(g) == value(w), f"{where}: {name} = {value(g)}, the model has {value(w)}"
            assert g == list(w), f"{where}: {name}: the value is the model's, the limbs are not: {g} / {list(w)}"
        if cut == "exit":
            assert max(max(g) for g in got) <= MASK and all(v < 2 * P for v in vals), f"{where}: not normalized below 2 N"
        else:
            assert _within(vals), f"{where}: a coordinate above the bounds table: {[v * 100 // P / 100 for v in vals]}"
            assert max(max(g) for g in got) < (1 << 29) + 32, f"{where}: a limb above 2^29 + 32"      # (no cut ends on `acc = operand`)
        X, Y, ZZ, ZZZ = (v % P for v in vals)
        assert ZZ and ZZZ, f"{where}: infinity"
        assert (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))) == G1.mul(G1_GEN, scalar), f"{where}: wrong point"
    return n

