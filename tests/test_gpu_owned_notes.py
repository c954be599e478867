"""GPU parity: owned notes -- og_note_seal_owned_batch_d, og_note_scan_owned_batch_d -- against tests/owned_note_spec.py; cases in
tests/owned_note_cases.py."""
import pytest

from tests import owned_note_cases as oc

pytestmark = pytest.mark.gpu

SIZES, REUSE = (0, 1, 63, 64, 65, 4097), (4097, 65)


def test_seal_owned(ctx):
    """memos and notes byte for byte, every refusal of the ordinary seal on its own"""
    oc.case_seal(ctx)


def test_scan_owned(ctx):
    """every class of memo under scanning keys below, at and above l, with and without leaves; the two forms never see each other"""
    oc.case_scan(ctx)


def test_scan_owned_refuses_a_non_canonical_sk(ctx):
    oc.case_scan_refuses_a_non_canonical_sk(ctx)


@pytest.mark.parametrize("name", ("seal", "scan"))
def test_owned_shapes(ctx, name):
    """one lane to 65 waves, tiled from a prime-sized pool at two offsets, hits in lanes 0 and 63 and in the first and last wave; then
    a larger call followed by a smaller one, into a reused output buffer"""
    oc.case_shapes(ctx, name, SIZES, REUSE)
