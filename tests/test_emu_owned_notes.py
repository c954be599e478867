"""Owned notes on the CPU interpreter (tests/hipemu): sealing and scanning; cases in tests/owned_note_cases.py, the scheme in
tests/owned_note_spec.py."""
import pytest

from tests import owned_note_cases as oc

SIZES, REUSE = (0, 1, 64, 65, 129), (129, 65)


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_emu_seal_owned(ectx):
    """memos and notes byte for byte, every refusal of the ordinary seal on its own"""
    oc.case_seal(ectx)


def test_small_p_is_refused_by_the_spec():
    oc.case_small_p_is_refused_by_the_spec()


def test_emu_scan_owned(ectx):
    """every class of memo under scanning keys below, at and above l, with and without leaves; the two forms never see each other"""
    oc.case_scan(ectx)


def test_emu_scan_owned_refuses_a_non_canonical_sk(ectx):
    oc.case_scan_refuses_a_non_canonical_sk(ectx)


@pytest.mark.parametrize("name", ("seal", "scan"))
def test_emu_owned_shapes(ectx, name):
    oc.case_shapes(ectx, name, SIZES, REUSE)
