"""View keys on the CPU interpreter (tests/hipemu): sealing to (PV, PS), scanning with (v, PS), unlocking with sk; cases in
tests/view_note_cases.py, the scheme in tests/view_note_spec.py."""
import pytest

from tests import view_note_cases as vc

SIZES, REUSE = (0, 1, 64, 65, 129), (129, 65)


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_emu_seal_view(ectx):
    """memos and notes byte for byte, every refusal on its own"""
    vc.case_seal(ectx)


def test_small_p_is_refused_by_the_spec():
    vc.case_small_p_is_refused_by_the_spec()


def test_emu_scan_view(ectx):
    """every class of memo under view scalars below, at and above l, with and without leaves; the three forms never see each other"""
    vc.case_scan(ectx)


def test_emu_scan_view_refusals(ectx):
    vc.case_scan_refusals(ectx)


def test_emu_unlock(ectx):
    """sk + t past l every number of times, and every way not to unlock"""
    vc.case_unlock(ectx)


def test_emu_unlock_opens_what_scan_owned_opens(ectx):
    vc.case_unlock_opens_what_scan_owned_opens(ectx)


def test_emu_torsion_ps_never_unlocks(ectx):
    vc.case_torsion_ps_never_unlocks(ectx)


@pytest.mark.parametrize("name", ("seal", "scan", "unlock"))
def test_emu_view_shapes(ectx, name):
    vc.case_shapes(ectx, name, SIZES, REUSE)


def test_emu_the_view_key_cannot_spend(ectx):
    vc.case_the_view_key_cannot_spend(ectx, 2)


def test_emu_view_through_the_pool(ectx):
    vc.case_through_the_pool(ectx, 2)
