"""Chains of group additions at the edge of the weak-X invariant (owshen_amd/csrc/ec.hip.h) -- TEST INFRASTRUCTURE ONLY.

og_hook_ec_chain_d (hooks build) walks one chain per lane with xyzz_madd_signed_w / xyzz_add_w and NO normalisation in between,
from an accumulator handed in as raw limbs and back out as raw limbs.  The accumulators here start from a NON-CANONICAL X: the
Montgomery residue x plus j N for every admissible j (0..5; j = 5 with an x picked just under N / 2, i.e. X just under the 5.5N of
the invariant), in G2 per component; Y, ZZ, ZZZ likewise from [0, 2N).  A chain is 310 steps:
  * mixed additions of +-(m G) from a pool, q given as x or x + N;
  * q = the running point itself (the doubling branch) and q = its negative (the infinity branch), each followed by more additions;
  * q = infinity, as (0, 0) and as (N, 0); the first-entry path (accumulator at infinity);
or, in the `add` flavour, the same with full additions of XYZZ operands that carry their own non-canonical X and a ZZ != 1
(operand = the running point: the doubling with a weak X; operand = its negative; operand at infinity).
Every chain is also run CUT after 1, 2 and a few more steps (the rest padded with q = infinity, which returns the accumulator as it
is), so the intermediate accumulators are seen too, and once with xyzz_norm as the last step.

What is checked, with zero tolerance: the limbs that come back are normalized, X is below 5.5N (below 2N after xyzz_norm), Y, ZZ
and ZZZ are below 2N, and the affine point is the one oracle/py/curve computes for the same scalars."""
import ctypes as C
import functools
import random

import numpy as np

from oracle.py import fields
from oracle.py.curve import G1, G2, G1_GEN, G2_GEN

P, MASK, RR = fields.P, (1 << 29) - 1, 1 << 261
N_STEPS, REC = 310, 1 + 8 * 9
CUTS = (1, 2, 52, 102, 105, 200, N_STEPS)


def limbs(v):
    return [(v >> (29 * i)) & MASK for i in range(9)]


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


class _G:
    def __init__(self, group, gen, nf):
        self.group, self.gen, self.nf, self.F = group, gen, nf, group.F

    def comps(self, e):
        return [e] if self.nf == 1 else list(e)

    def elem(self, cs):
        return cs[0] if self.nf == 1 else tuple(cs)

    def scale(self, pt, lam):
        """the XYZZ form (x l^2, y l^3, l^2, l^3) of an affine point, or of infinity (ZZ = 0)"""
        F = self.F
        if pt is None:
            return (F.one, F.one, F.zero, F.zero)
        l2 = F.sqr(lam)
        l3 = F.mul(l2, lam)
        return (F.mul(pt[0], l2), F.mul(pt[1], l3), l2, l3)

    def rand_elem(self, rnd):
        return self.elem([rnd.randrange(1, P) for _ in range(self.nf)])


GROUPS = {1: _G(G1, G1_GEN, 1), 2: _G(G2, G2_GEN, 2)}


def mont(c):
    return c * RR % P


def fe_words(c, j):
    """limbs of the Montgomery residue of c plus j N"""
    return limbs(mont(c) + j * P)


def _pick_lambda(g, pt, rnd, j):
    """a scaling whose X residue admits x + j N < 5.5 N in every component -- for j = 5 the one among 400 draws whose largest
    component is largest, i.e. an X (in G2: one component of it) just under the bound"""
    best, best_v = None, -1
    for _ in range(400 if j == 5 else 1):
        lam = g.rand_elem(rnd)
        xs = [mont(c) for c in g.comps(g.scale(pt, lam)[0])]
        if j < 5:
            return lam
        if all(2 * x < P for x in xs) and max(xs) > best_v:
            best, best_v = lam, max(xs)
    assert best is not None
    return best


def _xyzz_words(g, q, jx, rnd):
    """XYZZ as raw limbs: X + jx N, the other coordinates from [0, 2N)"""
    out = []
    for k, e in enumerate(q):
        for c in g.comps(e):
            out += fe_words(c, jx if k == 0 else rnd.randrange(2))
    return out


@functools.lru_cache(None)
def build(gid):
    """-> (acc words [n, 4 W], step words [n, N_STEPS, REC], expectations [(scalar or None, normed)], W)"""
    g = GROUPS[gid]
    rnd = random.Random(f"ec_chain/{gid}")
    W = g.nf * 9
    pool = [(m, g.group.mul(g.gen, m)) for m in (rnd.randrange(1, fields.R) for _ in range(24))]
    accs, steps, expect = [], [], []

    def affine_rec(pt, kind, xn=0):
        rec = [kind] + [0] * (REC - 1)
        if pt is not None:
            w = []
            for e in pt:
                for c in g.comps(e):
                    w += fe_words(c, rnd.randrange(2))
            rec[1:1 + len(w)] = w
        elif xn:
            rec[1:10] = limbs(P)          # x = N, y = 0: infinity all the same
        return rec

    for flavour in ("madd", "add"):
        for j in range(6):
            a = rnd.randrange(1, fields.R)
            apt = g.group.mul(g.gen, a)
            lam = _pick_lambda(g, apt, rnd, j)
            acc_words = _xyzz_words(g, g.scale(apt, lam), j, rnd)
            s, recs, at = a, [], []
            for t in range(N_STEPS):
                cur = None if s is None else g.group.mul(g.gen, s) if t in (50, 100) else None
                if flavour == "madd":
                    if t == 50:                                   # q = acc: the doubling branch
                        recs.append(affine_rec(cur, 0)); s = 2 * s % fields.R
                    elif t == 100:                                # q = -acc (as +acc with the sign bit): infinity
                        recs.append(affine_rec(cur, 1)); s = None
                    elif t in (101, 160):                         # q = infinity
                        recs.append(affine_rec(None, t & 1, xn=t == 160))
                    else:                                         # t = 102: the first-entry path
                        m, pt = pool[rnd.randrange(len(pool))]
                        neg = rnd.randrange(2)
                        recs.append(affine_rec(pt, neg))
                        s = ((s or 0) + (-m if neg else m)) % fields.R
                else:
                    rec = [2] + [0] * (REC - 1)
                    if t == 50:                                   # operand = acc under another scaling: xyzz_dbl of a weak X
                        op, ds = cur, s
                    elif t == 100:
                        op, ds = g.group.neg(cur), None
                    elif t in (101, 160):
                        op, ds = None, 0
                    else:
                        m, pt = pool[rnd.randrange(len(pool))]
                        op, ds = pt, m
                    jx = rnd.randrange(5)
                    w = _xyzz_words(g, g.scale(op, _pick_lambda(g, op, rnd, jx) if op is not None else g.F.one), jx if op is not None else 0, rnd)
                    rec[1:1 + len(w)] = w
                    recs.append(rec)
                    s = None if ds is None else ((s or 0) + ds) % fields.R if (s is not None or ds) else None
                at.append(s)
            pad = affine_rec(None, 0)
            for cut in CUTS + ("norm",):
                n = N_STEPS - 1 if cut == "norm" else cut
                accs.append(acc_words)
                steps.append(recs[:n] + ([[3] + [0] * (REC - 1)] if cut == "norm" else []) + [pad] * (N_STEPS - n - (cut == "norm")))
                expect.append((at[n - 1], cut == "norm", flavour, j, cut))
    return (np.array(accs, dtype=np.uint64).astype(np.uint32), np.array(steps, dtype=np.uint64).astype(np.uint32), expect, W)


def run(ctx, gid):
    """one launch of og_hook_ec_chain_d over every chain of the group; returns the number of chains checked"""
    g = GROUPS[gid]
    accs, steps, expect, W = build(gid)
    n = len(expect)
    assert steps.shape == (n, N_STEPS, REC) and accs.shape == (n, 4 * W)
    fn = ctx._lib.og_hook_ec_chain_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    d_acc, d_steps = ctx.to_device(accs), ctx.to_device(steps)
    d_out = ctx.empty(n * 4 * W * 4)
    ctx._pre()
    ctx._check(fn(ctx._h, gid - 1, ctx.ptr(d_acc), ctx.ptr(d_steps), n, N_STEPS, ctx.ptr(d_out)))
    out = np.asarray(ctx.to_host(d_out)).view(np.uint32).reshape(n, 4, g.nf, 9)
    seen_weak = 0
    for k, (s, normed, flavour, j, cut) in enumerate(expect):
        where = f"group {gid} {flavour} chain j={j} cut={cut}"
        assert int(out[k].max()) <= MASK, f"{where}: limbs not normalized"
        v = [[value(out[k, c, f]) for f in range(g.nf)] for c in range(4)]
        assert all(2 * x < (4 if normed else 11) * P for x in v[0]), f"{where}: X above {'2N' if normed else '5.5N'}"
        assert all(x < 2 * P for c in (1, 2, 3) for x in v[c]), f"{where}: Y / ZZ / ZZZ above 2N"
        seen_weak += any(x >= 2 * P for x in v[0])
        X, Y, ZZ, ZZZ = (g.elem([x % P for x in c]) for c in v)
        if s is None or s == 0:
            assert g.F.is_zero(ZZ), f"{where}: expected the point at infinity"
            continue
        assert not g.F.is_zero(ZZ), f"{where}: unexpected infinity"
        got = (g.F.mul(X, g.F.inv(ZZ)), g.F.mul(Y, g.F.inv(ZZZ)))      # the Montgomery factors cancel
        assert got == g.group.mul(g.gen, s), f"{where}: wrong point"
    assert seen_weak > n // 4, "the chains never left X above 2N: the weak invariant was not exercised"
    return n
