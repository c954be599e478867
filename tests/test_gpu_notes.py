"""GPU parity: stealth notes -- og_note_seal_batch_d, og_note_scan_batch_d and the uniform-scalar seam -- against tests/note_spec.py;
cases in tests/note_cases.py.  The seam exists in the hooks build only."""
import pytest

from tests import note_cases as nc

pytestmark = pytest.mark.gpu

SIZES, REUSE = (0, 1, 63, 64, 65, 4097), (4097, 65)


def test_mul_uniform_seam(ctx_hooks):
    """s P for one scalar over all lanes = multiply(P, s): the recoding's edges over BASE, the identity, the eight small points, a
    mixed-order point and random points (og_hook_ed_mul_uniform_d)"""
    nc.case_mul_uniform(ctx_hooks)


def test_seal(ctx):
    """memos and notes byte for byte, every refusal on its own"""
    nc.case_seal(ctx)


def test_scan(ctx):
    """every class of memo under four scanning keys, with and without leaves, with and without the opened rows"""
    nc.case_scan(ctx)


def test_scan_refuses_a_non_canonical_sk(ctx):
    nc.case_scan_refuses_a_non_canonical_sk(ctx)


@pytest.mark.parametrize("name", ("seal", "scan"))
def test_shapes(ctx, name):
    """one lane to 65 waves, tiled from a prime-sized pool at two offsets, hits in lanes 0 and 63 and in the first and last wave; then
    a larger call followed by a smaller one"""
    nc.case_shapes(ctx, name, SIZES, REUSE)


def test_through_the_pool(ctx):
    """seal -> transfer (pay_leaf = the sealed leaf) -> append -> scan -> withdraw the opened note -> og_verify, depth 2"""
    nc.case_through_the_pool(ctx)
