"""The send statement on the CPU interpreter (tests/hipemu); cases in tests/send_cases.py.  The statement has one walk, the lane-local
kernel k_send_core, whatever the size of the call."""
import pytest

from tests import send_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_send_r1cs_and_witness_match_spec(ectx, depth):
    cases.case_send_r1cs_and_witness_match_spec(ectx, depth, n=7)


def test_emu_send_end_to_end(ectx):
    cases.case_send_end_to_end(ectx, 2, n=2)


def test_emu_send_forgeries_are_unprovable(ectx):
    cases.case_send_forgeries_are_unprovable(ectx, 2)


def test_emu_one_spent_set(ectx):
    cases.case_one_spent_set(ectx, 2)


def test_emu_send_the_theft_is_closed(ectx):
    cases.case_send_the_theft_is_closed(ectx, 2)


def test_emu_send_record_boundary(ectx):
    cases.case_send_record_boundary(ectx, 2)


def test_emu_send_second_slab(ectx):
    cases.case_send_second_slab(ectx, 2)


def test_emu_two_hops_with_no_claim(ectx):
    cases.case_two_hops_with_no_claim(ectx, 3)
