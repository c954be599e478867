"""The redeem statement on the GPU through the C ABI; cases in tests/redeem_cases.py.  Shapes: depth 2 and the deployed depth 32; calls
of 1, 5, 65 (past one wave, a ragged second one) and 130 requests; one depth-32 key serves the module."""
import pytest

from tests import redeem_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases.key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 1), (2, 5), (2, 65), (2, 130), (32, 5), (32, 65)])
def test_redeem_r1cs_and_witness_match_spec(ctx, depth, n):
    cases.case_redeem_r1cs_and_witness_match_spec(ctx, depth, n=n)


@pytest.mark.parametrize("n", [1, 4])
def test_redeem_end_to_end_depth2(ctx, n):
    cases.case_redeem_end_to_end(ctx, 2, n=n)


def test_redeem_end_to_end_depth32(ctx, key32):
    cases.case_redeem_end_to_end(ctx, 32, n=2, key=key32)


def test_redeem_batch_130_verifies_depth32(ctx, key32):
    cases.case_redeem_batch_130_verifies(ctx, 32, key32)


def test_redeem_forgeries_are_unprovable(ctx):
    cases.case_redeem_forgeries_are_unprovable(ctx, 2)


def test_redeem_forgeries_are_unprovable_depth32(ctx, key32):
    cases.case_redeem_forgeries_are_unprovable(ctx, 32, key=key32)


def test_redeem_the_theft_is_closed(ctx):
    cases.case_redeem_the_theft_is_closed(ctx, 2)


def test_redeem_record_boundary(ctx):
    cases.case_redeem_record_boundary(ctx, 2)


def test_redeem_second_slab(ctx_hooks):
    cases.case_redeem_second_slab(ctx_hooks, 2)
