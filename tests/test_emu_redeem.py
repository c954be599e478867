"""The redeem statement on the CPU interpreter (tests/hipemu); cases in tests/redeem_cases.py.  The statement has one walk, the
lane-local kernel k_redeem_core, whatever the size of the call."""
import pytest

from tests import redeem_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_redeem_r1cs_and_witness_match_spec(ectx, depth):
    cases.case_redeem_r1cs_and_witness_match_spec(ectx, depth, n=7)


def test_emu_redeem_end_to_end(ectx):
    cases.case_redeem_end_to_end(ectx, 2, n=2)


def test_emu_redeem_forgeries_are_unprovable(ectx):
    cases.case_redeem_forgeries_are_unprovable(ectx, 2)


def test_emu_redeem_the_theft_is_closed(ectx):
    cases.case_redeem_the_theft_is_closed(ectx, 2)


def test_emu_redeem_record_boundary(ectx):
    cases.case_redeem_record_boundary(ectx, 2)


def test_emu_redeem_second_slab(ectx):
    cases.case_redeem_second_slab(ectx, 2)
