"""The raw-limb case table of tests/field_raw_cases.py on the CPU interpreter: the HOST form of every routine (the MontCols column
walk, what og_verify runs) through the same entry point the GPU test uses, og_hook_fe_raw_d of the hooks build -- one list of
cases, one big-integer reference for the host walk and the device asm.  Plus the table's own coverage test, which needs neither."""
import pytest

from tests import field_raw_cases as frc


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name,field", frc.PARAMS)
def test_table_holds_every_extreme_class_in_every_position(name, field):
    """for every op, operand position and named extreme class a profile admits there, at least one case has THAT position hold
    THAT class, with the partners cycling through their own classes; every case meets the routine's documented contract"""
    op, N, cases = frc.OPS[name], frc.MODS[field], frc.table(name, field)
    have = {}
    for case in cases:
        assert len(case.limbs) == op.arity == len(case.classes)
        op.contract(case.limbs, N)
        for pos, (c, l) in enumerate(zip(case.classes, case.limbs)):
            have.setdefault((pos, c), set()).add(tuple(x for q, x in enumerate(case.classes) if q != pos))
            if c in frc.CLASSES:      # the class is what its name says: limb width and value bound
                assert len(l) == 9 and 0 <= min(l) and max(l) < 1 << frc.CLASSES[c][2] and frc.value(l) <= frc.CLASSES[c][1] * N
    need = frc.required_coverage(name)
    assert need or op.extra
    for _, pos, c in need:
        assert (pos, c) in have, f"{name}: no case with class {c} in position {pos}"
        if op.arity > 1 and op.reps > 1:
            assert len(have[(pos, c)]) > 1, f"{name}: the partners of {c} in position {pos} never change"
    assert 100 <= len(cases) <= 5000 or name == "fe_inv"
    assert cases is frc.table(name, field)      # built once, shared by every test that runs it


def test_the_classes_the_issue_names_are_in_the_table():
    names = {c for name, f in frc.PARAMS for case in frc.table(name, f) for c in case.classes}
    for must in ("zero", "one", "N-1", "N", "N+1", "top2", "top2-1", "sat2", "low8sat", "2^253-1", "lazy8_rand", "lazy31_worst",
                 "top6", "sat6", "top10", "sat10", "rand2"):
        assert must in names, must
    # the all-limbs-at-2^31 operand in EITHER position of fe_mul
    for f in (0, 1):
        pos = {case.classes.index("lazy31_worst") for case in frc.table("fe_mul", f) if "lazy31_worst" in case.classes}
        assert pos == {0, 1}


@pytest.mark.parametrize("name,field", frc.PARAMS)
def test_emu_field_raw(ectx, name, field):
    frc.run(ectx, name, field)
