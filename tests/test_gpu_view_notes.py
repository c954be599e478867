"""GPU parity: view keys -- og_note_seal_view_batch_d, og_note_scan_view_batch_d, og_note_unlock_batch_d -- against
tests/view_note_spec.py; cases in tests/view_note_cases.py."""
import pytest

from tests import view_note_cases as vc

pytestmark = pytest.mark.gpu

SIZES, REUSE = (0, 1, 63, 64, 65, 4097), (4097, 65)


def test_seal_view(ctx):
    """memos and notes byte for byte, every refusal on its own"""
    vc.case_seal(ctx)


def test_scan_view(ctx):
    """every class of memo under view scalars below, at and above l, with and without leaves; the three forms never see each other"""
    vc.case_scan(ctx)


def test_scan_view_refusals(ctx):
    vc.case_scan_refusals(ctx)


def test_unlock(ctx):
    """sk + t past l every number of times, and every way not to unlock"""
    vc.case_unlock(ctx)


def test_unlock_opens_what_scan_owned_opens(ctx):
    vc.case_unlock_opens_what_scan_owned_opens(ctx)


def test_torsion_ps_never_unlocks(ctx):
    vc.case_torsion_ps_never_unlocks(ctx)


@pytest.mark.parametrize("name", ("seal", "scan", "unlock"))
def test_view_shapes(ctx, name):
    """one lane to 65 waves, tiled from a prime-sized pool at two offsets, hits in lanes 0 and 63 and in the first and last wave; then
    a larger call followed by a smaller one, into a reused output buffer"""
    vc.case_shapes(ctx, name, SIZES, REUSE)


def test_the_view_key_cannot_spend(ctx):
    vc.case_the_view_key_cannot_spend(ctx, 2)


def test_view_through_the_pool(ctx):
    vc.case_through_the_pool(ctx, 2)
