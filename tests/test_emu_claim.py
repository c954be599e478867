"""The claim statement on the CPU interpreter (tests/hipemu); cases in tests/claim_cases.py.  The statement has one walk, the
lane-local kernel k_claim_core, whatever the size of the call."""
import pytest

from tests import claim_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_claim_r1cs_and_witness_match_spec(ectx, depth):
    cases.case_r1cs_and_witness_match_spec(ectx, depth, n=5)


def test_emu_claim_end_to_end(ectx):
    cases.case_claim_end_to_end(ectx, 2, n=2)


def test_emu_claim_forgeries_are_unprovable(ectx):
    cases.case_forgeries_are_unprovable(ectx, 2)


def test_emu_claim_the_theft_is_closed(ectx):
    cases.case_the_theft_is_closed(ectx, 2)


def test_emu_claim_record_boundary(ectx):
    cases.case_record_boundary(ectx, 2)


def test_emu_claim_second_slab(ectx):
    cases.case_second_slab(ectx, 2)


def test_emu_claim_through_the_pool(ectx):
    cases.case_through_the_pool(ectx, 2)
