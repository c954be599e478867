"""The split statement on the CPU interpreter (tests/hipemu); cases in tests/split_cases.py."""
import pytest

from tests import split_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_split_r1cs_and_witness_match_spec(ectx, depth):
    cases.case_r1cs_and_witness_match_spec(ectx, depth, n=4)


def test_emu_split_end_to_end(ectx):
    cases.case_split_end_to_end(ectx, 2, n=2)


def test_emu_split_overdraw_is_unprovable(ectx):
    cases.case_overdraw_is_unprovable(ectx, 2)


def test_emu_split_record_boundary(ectx):
    cases.case_record_boundary(ectx, 2)
