"""GPU parity: batched BabyJubJub EdDSA verification with the MiMC7 sponge; cases in tests/eddsa_cases.py."""
import pytest

pytestmark = pytest.mark.gpu


def test_eddsa_batch(ctx):
    from tests import eddsa_cases
    eddsa_cases.case_eddsa_batch(ctx, n_valid=40, seed=7)


def test_eddsa_edges(ctx):
    """the identity, points of order 2, 4 and 8, pk = +-BASE, s outside the subgroup range, sign flips, an off-curve R and every
    field non-canonical, in one call; both references decide every canonical record"""
    from tests import eddsa_cases
    eddsa_cases.case_eddsa_edges(ctx)


def test_eddsa_shapes(ctx):
    """0 .. 257 workgroups with ragged last waves, tiled from a pool of 193 decided records; then 16 385, 65, 16 385 again at
    another offset over the one reused result buffer"""
    from tests import eddsa_cases
    eddsa_cases.case_eddsa_shapes(ctx, (0, 1, 63, 64, 65, 127, 128, 129, 16385), reuse=(16385, 65, 16385))
