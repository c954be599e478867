"""The key blobs at their consumers on the GPU through the C ABI; cases in tests/key_blob_cases.py.  Everything at toy size: a
25-constraint key whose sections end off every 32-byte boundary, and the smallest key there is (domain 2, no private wire)."""
import pytest

from tests import key_blob_cases as cases

pytestmark = pytest.mark.gpu


def test_k1_meets_every_padding(ctx):
    cases.case_k1_meets_every_padding(ctx)


@pytest.mark.parametrize("consumer", cases.PK_CONSUMERS)
def test_outcomes_of_malformed_proving_keys(ctx, consumer):
    cases.case_outcomes(ctx, "pk", consumer)


@pytest.mark.parametrize("consumer", cases.VK_CONSUMERS)
def test_outcomes_of_malformed_verifying_keys(ctx, consumer):
    cases.case_outcomes(ctx, "vk", consumer)


def test_blob_digests(ctx):
    cases.case_digests(ctx)


@pytest.mark.parametrize("consumer", sorted(cases.CALLS))
def test_unaligned_blobs(ctx, consumer):
    cases.case_unaligned(ctx, consumer)


def test_pk_info_is_the_header(ctx):
    cases.case_pk_info(ctx)
