"""The routines of the single-Q addition on the CPU interpreter: the HOST column walk of fe_sqr_plus / fe_sqr_add_plus and the
limb-wise helpers beside them, through og_hook_fe_raw_d, on the cases of tests/field_rider_cases.py; plus that table's own
coverage test (every named extreme class in every position it is admitted to)."""
import pytest

from tests import field_raw_cases as frc
from tests import field_rider_cases as rider


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name,field", rider.PARAMS)
def test_table_holds_every_extreme_class_in_every_position(name, field):
    op, N, cases = frc.OPS[name], frc.MODS[field], frc.table(name, field)
    have = set()
    for case in cases:
        assert len(case.limbs) == op.arity == len(case.classes)
        op.contract(case.limbs, N)
        for pos, (c, l) in enumerate(zip(case.classes, case.limbs)):
            have.add((pos, c))
            assert len(l) == 9 and 0 <= min(l) and max(l) < 1 << frc.CLASSES[c][2] and 10 * frc.value(l) <= round(10 * frc.CLASSES[c][1]) * N
    need = frc.required_coverage(name)
    assert need
    for _, pos, c in need:
        assert (pos, c) in have, f"{name}: no case with class {c} in position {pos}"
    assert 100 <= len(cases) <= 5000


def test_the_budget_and_the_addend_are_reached():
    """the squared operand at 12.9 N (166 of the 169 N^2), a^2 + c d at 164 N^2, the addend with limbs above 2^30"""
    for f in (0, 1):
        N = frc.MODS[f]
        assert max(frc.value(c.limbs[0]) ** 2 for c in frc.table("fe_sqr_plus", f)) > 166 * N * N
        assert max(frc.value(c.limbs[0]) ** 2 + frc.value(c.limbs[1]) * frc.value(c.limbs[2]) for c in frc.table("fe_sqr_add_plus", f)) > 163 * N * N
        assert max(max(c.limbs[1]) for c in frc.table("fe_sqr_plus", f)) >= 1 << 30
        assert max(max(c.limbs[3]) for c in frc.table("fe_sqr_add_plus", f)) >= 1 << 30


@pytest.mark.parametrize("name,field", rider.PARAMS)
def test_emu_field_rider(ectx, name, field):
    frc.run(ectx, name, field)
