"""The join statement on the CPU interpreter (tests/hipemu); cases in tests/join_cases.py."""
import pytest

from tests import join_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_join_r1cs_and_witness_match_spec(ectx, depth):
    cases.case_r1cs_and_witness_match_spec(ectx, depth, n=5)


def test_emu_join_end_to_end(ectx):
    cases.case_join_end_to_end(ectx, 2, n=2)


def test_emu_join_forgeries_are_unprovable(ectx):
    cases.case_forgeries_are_unprovable(ectx, 2)


def test_emu_join_different_roots(ectx):
    cases.case_different_roots(ectx, 2)


def test_emu_join_record_boundary(ectx):
    cases.case_record_boundary(ectx, 2)
