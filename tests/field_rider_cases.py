"""Raw-limb cases for the routines the single-Q addition added to field.hip.h / ec.hip.h -- TEST INFRASTRUCTURE ONLY.

Built the way tests/field_raw_cases.py builds its table, and ON it: the ops below join frc.OPS under new names (op numbers 37..41
and 71..74 of og_hook_fe_raw_d), so frc.table / frc.run / frc.check serve them unchanged -- same three views (the host column
walk, the asm text on Python integers, the hardware), same big-integer reference, zero tolerance.  frc.PARAMS, which the older
tests are parametrised over, was fixed when frc was imported and does not see them.

New operand classes:
* the addend of the squaring-plus-addend forms ("rider", fe_rider4): 4N - a - 2b limb-wise against 4N with every limb below the
  top inflated by 3 x 2^29 -- limbs up to 2^31, value in (0, 4N];
* the weak X of the group law: normalized limbs, top limb at most that of 6N less the unit it lent (fe_neg_lazy6);
* a squared operand at the top of the 169 N^2 budget (12.9 N)."""
from tests import field_raw_cases as frc
from tests.field_raw_cases import CLASSES, MASK, DBL, L4, L8, N2, W4, W6, W8, W10, limbs, lazy_neg, mont, value

_HALF = ["zero", "one", "low8sat", "ridb_top", "ridb_sat", "ridb_rand"]   # b of fe_rider4: a + 2b stays below 4N - 2^234


def rider(a, b, N):
    """4N - a - 2b limb-wise, from the definition (not from the constants of field.hip.h)"""
    n4 = limbs(4 * N)
    return [n4[j] + (3 << 29 if j < 8 else 0) - (3 if j > 0 else 0) - a[j] - 2 * b[j] for j in range(9)]


def _ridb_top(N):
    """the largest top limb b may have beside an a < 2N"""
    return (limbs(4 * N)[8] - 3 - limbs(2 * N - 1)[8]) // 2


CLASSES["ridb_top"] = (lambda N, rng: [0] * 8 + [_ridb_top(N)], 1, 29)
CLASSES["ridb_sat"] = (lambda N, rng: [MASK] * 8 + [_ridb_top(N) - 1], 1, 29)
CLASSES["ridb_rand"] = (lambda N, rng: [rng.randrange(1 << 29) for _ in range(8)] + [rng.randrange(_ridb_top(N))], 1, 29)
CLASSES["rid_of_0"] = (lambda N, rng: rider(limbs(0), limbs(0), N), 4, 31)                                  # the constant: the largest limbs
CLASSES["rid_low"] = (lambda N, rng: rider([MASK] * 8 + [0], [MASK] * 8 + [0], N), 4, 31)                   # every low limb at its least
CLASSES["rid_top"] = (lambda N, rng: rider(limbs(2 * N - 1), [MASK] * 8 + [_ridb_top(N) - 1], N), 4, 31)    # the least value
CLASSES["rid_rand"] = (lambda N, rng: rider(limbs(rng.randrange(2 * N)), CLASSES["ridb_rand"][0](N, rng), N), 4, 31)
CLASSES["top12.9"] = (lambda N, rng: limbs(129 * N // 10 - 1), 12.9, 29)
CLASSES["sat12.9"] = (lambda N, rng: limbs((((129 * N // 10) >> 232) - 1) << 232 | ((1 << 232) - 1)), 12.9, 29)
CLASSES["rand12.9"] = (lambda N, rng: limbs(rng.randrange(129 * N // 10)), 12.9, 29)
CLASSES["rand6s"] = (lambda N, rng: limbs(rng.randrange(((6 * N) >> 232) << 232)), 6, 29)
CLASSES["weak5.5"] = (lambda N, rng: limbs(11 * N // 2 - 1), 6, 29)                                       # the weak invariant's edge
for _k in (2, 4):
    CLASSES[f"{_k}N"] = (lambda N, rng, k=_k: limbs(k * N), _k, 29)
    CLASSES[f"{_k}N+1"] = (lambda N, rng, k=_k: limbs(k * N + 1), _k + 1, 29)

RID = ["rid_of_0", "rid_low", "rid_top", "rid_rand"]
W13 = ["top12.9", "sat12.9", "rand12.9"]
S6 = ["sat6", "weak5.5", "rand6s"]
NORM6 = ["2N", "2N+1", "top4", "4N", "4N+1", "top6", "top6-1", "sat6", "weak5.5", "rand6"]


def _rider_contract(op):
    def contract(ls, N):
        v = [value(l) for l in ls]
        lazy = 0
        for term in op.terms:
            if term[0] == "sqr":
                assert max(ls[term[1]]) <= MASK, "the squared operand is normalized"
            else:
                wide = [l for l in (ls[term[1]], ls[term[2]]) if max(l) > MASK]
                assert len(wide) <= 1 and all(max(l) < 1 << 30 for l in wide)
                lazy += len(wide)
        assert lazy <= op.max_lazy
        assert frc._product_total(op, v) < 169 * N * N
        assert 0 <= min(ls[op.plus]) and max(ls[op.plus]) < 1 << 31 and 0 < v[op.plus] <= 4 * N
    return contract


def _fq2(name, num, arity, profiles, bounds, comps, negated, plus, bound):
    """comps(v, N) -> the two sums of products (None: no product); plus(v, N, k) -> what component k adds to its reduction"""
    def ref(ls, N):
        v = [value(l) for l in ls]
        out = []
        for k, tot in enumerate(comps(v, N)):
            r = 0
            if tot is not None:
                assert tot < 169 * N * N
                r = mont(tot, N)
                assert r < 2 * N
            out += limbs(r + plus(v, N, k))
        return out
    op = frc.Op(name, num, arity, profiles, ref, fields=(1,), out_fe=2, bound=bound)

    def contract(ls, N):
        frc._norm_contract(bounds)(ls, N)
        for pos, k in negated:
            assert ls[pos][8] < limbs(k * N)[8]
        for k in (0, 1):
            assert plus([value(l) for l in ls], N, k) >= 0
    op.contract = contract
    return op


def _build():
    ops = []
    sp = frc._product_op("fe_sqr_plus", 37, 2, [(N2, RID), (W6, RID), (W13, RID)], [("sqr", 0)], plus=1, asm="SQR_PLUS", max_lazy=0)
    sap = frc._product_op("fe_sqr_add_plus", 38, 4, [(N2, N2, N2, RID), (W6, L8, W6, RID), (W10, L8, W8, RID), (W8, DBL, W8, RID), (W6, L4, W10, RID)],
                          [("sqr", 0), ("mul", 1, 2)], plus=3, asm="SQR_ADD_PLUS", max_lazy=1)
    for op in (sp, sap):
        op.contract = _rider_contract(op)
        ops.append(op)
    n6 = frc._simple_op("fe_neg_lazy6", 39, [(N2,), (W4,), (S6,)], (6,), lambda v, ls, N: lazy_neg(6, ls[0], N), reps=1, n_random=200)
    n6.contract = lambda ls, N: frc._assert(max(ls[0]) <= MASK and ls[0][8] < limbs(6 * N)[8])
    ops.append(n6)
    r4 = frc._simple_op("fe_rider4", 40, [(N2, _HALF)], (2, 1), lambda v, ls, N: rider(ls[0], ls[1], N))
    r4.contract = lambda ls, N: frc._assert(max(max(l) for l in ls) <= MASK and ls[0][8] + 2 * ls[1][8] <= limbs(4 * N)[8] - 3)
    ops.append(r4)

    def norm_ref(v, ls, N):
        x = v[0] - 4 * N if v[0] >= 4 * N else v[0]
        return limbs(x - 2 * N if x >= 2 * N else x)
    ops.append(frc._simple_op("fe_norm_weak", 41, [(N2,), (NORM6,)], (6,), norm_ref, bound=2, reps=1, n_random=200))
    # -- the Fq2 forms of ec.hip.h (an Fq2 operand is two positions) --
    n8 = lambda x, N: 8 * N - x
    n4 = lambda x, N: 4 * N - x
    mm = lambda v, N: (v[0] * v[2] + n8(v[1], N) * v[3], v[0] * v[3] + v[1] * v[2])
    ops.append(_fq2("f_mul_minus6", 71, 6, [(N2,) * 6, (N2, N2, N2, N2, S6, S6)], (2, 2, 2, 2, 6, 6), mm, [(1, 8), (4, 6), (5, 6)],
                    lambda v, N, k: 6 * N - v[4 + k], 8))
    ops.append(_fq2("f_mul_n4", 72, 4, [(N2,) * 4, (N2, N2, W8, W8)], (2, 2, 8, 8),
                    lambda v, N: (v[0] * v[2] + n4(v[1], N) * v[3], v[0] * v[3] + v[1] * v[2]), [(1, 4)], lambda v, N, k: 0, 2))
    ops.append(_fq2("f_sqr_rider", 73, 6, [(N2, N2, N2, N2, _HALF, _HALF), (W6, W6, N2, N2, _HALF, _HALF)], (6, 6, 2, 2, 1, 1),
                    lambda v, N: (v[0] ** 2 + n8(v[1], N) * v[1], 2 * v[0] * v[1]), [(1, 8)], lambda v, N, k: 4 * N - v[2 + k] - 2 * v[4 + k], 6))
    ops.append(_fq2("f_q_minus", 74, 4, [(N2,) * 4, (N2, N2, S6, S6)], (2, 2, 6, 6), lambda v, N: (None, None), [(2, 6), (3, 6)],
                    lambda v, N, k: v[k] + 6 * N - v[2 + k], 8))
    return ops


OPS = {op.name: op for op in _build()}
assert not set(OPS) & set(frc.OPS) and not {op.num for op in OPS.values()} & {op.num for op in frc.OPS.values()}
frc.OPS.update(OPS)
PARAMS = [(name, f) for name, op in OPS.items() for f in op.fields]
