"""The send statement on the GPU through the C ABI; cases in tests/send_cases.py.  Shapes: depth 2 and the deployed depth 32; calls of
1, 5, 65 (past one wave, a ragged second one) and 130 requests; one depth-32 key serves the module."""
import pytest

from tests import send_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases.key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 1), (2, 5), (2, 65), (2, 130), (32, 5), (32, 65)])
def test_send_r1cs_and_witness_match_spec(ctx, depth, n):
    cases.case_send_r1cs_and_witness_match_spec(ctx, depth, n=n)


@pytest.mark.parametrize("n", [1, 4])
def test_send_end_to_end_depth2(ctx, n):
    cases.case_send_end_to_end(ctx, 2, n=n)


def test_send_end_to_end_depth32(ctx, key32):
    cases.case_send_end_to_end(ctx, 32, n=2, key=key32)


def test_send_batch_130_verifies_depth32(ctx, key32):
    cases.case_send_batch_130_verifies(ctx, 32, key32)


def test_send_forgeries_are_unprovable(ctx):
    cases.case_send_forgeries_are_unprovable(ctx, 2)


def test_send_forgeries_are_unprovable_depth32(ctx, key32):
    cases.case_send_forgeries_are_unprovable(ctx, 32, key=key32)


def test_one_spent_set(ctx):
    cases.case_one_spent_set(ctx, 2)


def test_send_the_theft_is_closed(ctx):
    cases.case_send_the_theft_is_closed(ctx, 2)


def test_send_record_boundary(ctx):
    cases.case_send_record_boundary(ctx, 2)


def test_send_second_slab(ctx_hooks):
    cases.case_send_second_slab(ctx_hooks, 2)


def test_two_hops_with_no_claim(ctx):
    cases.case_two_hops_with_no_claim(ctx, 3)
