"""Key generation from a powers-of-tau file and the delta step on the GPU through the C ABI; cases in tests/ptau_cases.py.  Sizes
are the smallest at which each piece can still go wrong: domain 2 (one butterfly, no twiddle), 32 (a DFT inside one wave), 2^10
(the deposit circuit: several workgroups per stage), a 1 051-term column (several waves of terms, two levels of 32-term runs
before the final sum)."""
import pytest

from tests import ptau_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_constraints,n_pub,extra_power", [(1, 0, 0), (25, 3, 0), (25, 3, 2)])
def test_setup_ptau_equals_setup(ctx, n_constraints, n_pub, extra_power):
    cases.case_equals_setup_small(ctx, n_constraints, n_pub, extra_power)


def test_setup_ptau_equals_setup_on_the_deposit_circuit(ctx):
    cases.case_equals_setup_deposit(ctx)


def test_setup_ptau_long_and_empty_columns(ctx):
    cases.case_long_and_empty_columns(ctx)


def test_pk_contribute(ctx):
    cases.case_contribute_small(ctx)


def test_pk_contribute_on_the_deposit_key(ctx):
    cases.case_contribute_deposit(ctx)


def test_pk_contribute_to_an_imported_key(ctx):
    cases.case_contribute_imported(ctx)


def test_ptau_key_proves_and_verifies(ctx):
    cases.case_key_works(ctx, n=64)


def test_ptau_file_round_trip(ctx):
    cases.case_file_round_trip(ctx)


def test_setup_ptau_refusals(ctx):
    cases.case_refusals(ctx)
    cases.case_null_handles(ctx._lib)


def test_ptau_info(ctx):
    cases.case_info(ctx, ctx._lib)
