"""The two squaring-plus-addend sequences of mont_gfx950.inc (SQR_PLUS, SQR_ADD_PLUS: X3 of the single-Q addition), checked
without a GPU the way tests/test_mont_asm.py checks the other nine: the committed text is what tools/gen_mont_asm.py writes, and
the text executed on Python integers returns, limb for limb, what the big-integer reference of tests/field_rider_cases.py says --
with the addend at its widest (limbs up to 2^31) and the sum of products at the top of its budget.  The interpreter asserts that
no write of the 64-bit column accumulator overflows."""
import importlib.util
import os
import re

import pytest

from tests import field_raw_cases as frc
from tests import field_rider_cases as rider
from tests.test_mont_asm import M32, gen, limbs, run

ASM_OPS = {op.asm: op for op in rider.OPS.values() if op.asm}


def test_both_routines_have_cases():
    assert set(ASM_OPS) == set(gen.RIDER_ROUTINES) and not set(gen.RIDER_ROUTINES) & set(gen.ROUTINES)


def test_generated_file_is_current():
    text = open(gen.OUT).read()
    for name, (terms, plus) in gen.RIDER_ROUTINES.items():
        body = re.search(r"#define OG_MONT_ASM_%s \\\n((?:  \".*\n)+)" % name, text)
        assert body, name
        got = [re.match(r'"(.*?)(?:\\n\\t)?"', l.strip()).group(1) for l in body.group(1).splitlines()]
        assert got == gen.routine(terms, plus), f"{name}: mont_gfx950.inc is stale -- run python tools/gen_mont_asm.py"


@pytest.mark.parametrize("mod_name", ["Fq", "Fr"])
@pytest.mark.parametrize("name", list(gen.RIDER_ROUTINES))
def test_routine_on_the_rider_case_table(name, mod_name):
    op, field = ASM_OPS[name], 1 if mod_name == "Fq" else 0
    n_mod = frc.MODS[field]
    terms, plus = gen.RIDER_ROUTINES[name]
    names = sorted({t for term in terms for t in term[1:]}) + ["p"]   # operand order of the C++ routine
    assert plus and len(names) == op.arity and [t[0] for t in terms] == [t[0] for t in op.terms]
    ins = gen.routine(terms, plus)
    base = {"v30": 0xDEADBEEF, "v31": 0xDEADBEEF, "inv": (-pow(n_mod, -1, 1 << 29)) % (1 << 29)}
    for j in range(9):
        base[f"n{j}"], base[f"r{j}"] = limbs(n_mod)[j], 0xDEADBEEF
    for k, case in enumerate(frc.table(op.name, field)):
        regs = dict(base)
        for nm, l in zip(names, case.limbs):
            for j in range(9):
                regs[f"{nm}{j}"] = l[j]
            for j in range(8):
                regs[f"{nm}d{j}"] = (l[j] << 1) & M32
        run(ins, regs)
        assert [regs[f"r{j}"] for j in range(9)] == frc.expected(op.name, field, case)[:9], (name, mod_name, k, case.classes)


def _mads(name):
    terms, plus = {**gen.ROUTINES, **gen.RIDER_ROUTINES}[name]
    return sum(1 for i in gen.routine(terms, plus) if i.startswith("v_mad_u64_u32"))


def test_multiply_adds_of_the_single_q_addition_quoted_in_the_roofline_tooling():
    """tools/pmc_traffic.py prices `mad_issue_frac` with the multiply-adds of one mixed addition as ec.hip.h computes it now
    (xyzz_madd_signed_w): G1 = P, R (product + addend), PP (square), PPP, Q, X3 (square + addend), Y3 (two products), ZZ3, ZZZ3;
    G2 = the Fq2 forms of the same.  81 and 324 fewer than the form that multiplied X1 PP out twice."""
    g1 = 2 * _mads("MUL_PLUS") + _mads("SQR") + 2 * _mads("MUL") + _mads("SQR_PLUS") + _mads("MUL_ADD") + 2 * _mads("MUL")
    g2 = (2 * 2 * _mads("MUL_ADD_PLUS")                      # P, R
          + _mads("SQR_ADD") + _mads("MUL")                  # PP
          + 2 * 2 * _mads("MUL_ADD")                         # PPP, Q
          + _mads("SQR_ADD_PLUS") + _mads("MUL_PLUS")        # X3
          + 2 * _mads("MUL_ADD4")                            # Y3
          + 2 * 2 * _mads("MUL_ADD"))                        # ZZ3, ZZZ3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(root, "tools", "pmc_traffic.py"))
    pt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pt)
    assert pt.MADS_SINGLE_Q["accumulate_g1"] == (g1, 81) == (1491, 81)
    assert pt.MADS_SINGLE_Q["accumulate_g2"] == (g2, 162) == (4512, 162)
    assert (pt.MADS["accumulate_g1"][0] - g1, pt.MADS["accumulate_g2"][0] - g2) == (81, 324)


@pytest.mark.parametrize("mod_name", ["Fq", "Fr"])
def test_mul_add_holds_the_limb_wise_d_of_the_fq_addition(mod_name):
    """Y3 = R D + (8N - Y1) PPP in Fq takes D = Q + (6N - X3) limb-wise (ec.hip.h f_q_minus): limbs up to 2^29 + 2^30, wider than
    the 2^30 MUL_ADD documents for a lazy operand.  Its columns hold 9 (1.5 + 1) 2^59 + 9 2^58 + carry < 2^64: the text run on the
    widest such D (Q and 6N - X3 at their largest limbs) beside R at 6N, 8N - 0 and PPP at 2N -- the interpreter asserts that no
    accumulator write overflows -- returns the exact Montgomery value."""
    field = 1 if mod_name == "Fq" else 0
    N = frc.MODS[field]
    terms, plus = gen.ROUTINES["MUL_ADD"]
    ins = gen.routine(terms, plus)
    sat2 = frc.CLASSES["sat2"][0](N, None)
    ds = [[q + x for q, x in zip(qq, frc.lazy_neg(6, xx, N))]
          for qq in (sat2, limbs(2 * N - 1), [frc.MASK] * 8 + [0]) for xx in (limbs(0), [0] * 8 + [limbs(6 * N)[8] - 1], limbs(N))]
    assert max(max(d) for d in ds) > 1 << 30      # wider than a lazy operand: the case the comment above is about
    rs = [limbs(6 * N - 1), frc.CLASSES["sat6"][0](N, None), limbs(2 * N + 1)]
    base = {"v30": 0xDEADBEEF, "v31": 0xDEADBEEF, "inv": (-pow(N, -1, 1 << 29)) % (1 << 29)}
    for j in range(9):
        base[f"n{j}"], base[f"r{j}"] = limbs(N)[j], 0xDEADBEEF
    for d in ds:
        for r in rs:
            for c, e in ((frc.lazy_neg(8, limbs(0), N), limbs(2 * N - 1)), (frc.CLASSES["lazy_sat30"][0](N, None), sat2)):
                ops = {"a": r, "b": d, "c": c, "d": e}
                total = frc.value(r) * frc.value(d) + frc.value(c) * frc.value(e)
                assert total < 169 * N * N
                regs = dict(base)
                for nm, l in ops.items():
                    for j in range(9):
                        regs[f"{nm}{j}"] = l[j]
                run(ins, regs)
                assert [regs[f"r{j}"] for j in range(9)] == limbs(frc.mont(total, N))
