"""og_ptau_verify / og_pk_verify on the GPU through the C ABI; cases in tests/ptau_verify_cases.py.  Sizes are the smallest at
which each piece can still go wrong: power 1 (sums of one and two terms), 2 (an interior point that is not the ratio point), 5
(inside one wave), 7 (255 / 128 points: past one workgroup of the scalar kernel and one block of the digit sort), 10 with the
deposit key (12-bit windows, several workgroups everywhere)."""
import pytest

from tests import ptau_cases, ptau_verify_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("power", [1, 2, 5, 7])
def test_ptau_verify_accepts_a_ceremony(ctx, power):
    cases.case_valid_file(ctx, power)


@pytest.mark.parametrize("power,names", [(1, cases.ALL_TAMPERED), (2, cases.ALL_TAMPERED[:6]), (2, cases.ALL_TAMPERED[6:]), (5, cases.SIZE_TAMPERED),
                                         (7, cases.SIZE_TAMPERED)])
def test_ptau_verify_names_what_was_tampered_with(ctx, power, names):
    cases.case_tampered_files(ctx, power, names)


def test_ptau_verify_refusals(ctx):
    cases.case_file_refusals(ctx)
    cases.case_null_handles(ctx._lib)


@pytest.mark.parametrize("extra_power", [0, 2])
def test_pk_verify_accepts_the_keys_of_the_file(ctx, extra_power):
    cases.case_valid_keys(ctx, ptau_cases._small(25, 3), 125, extra_power)


def test_pk_verify_accepts_an_exported_and_imported_key(ctx):
    cases.case_exported_and_imported_key(ctx)


def test_pk_verify_foreign_keys(ctx):
    cases.case_foreign_keys(ctx)


@pytest.mark.parametrize("part", [0, 1, 2])
def test_pk_verify_names_what_was_tampered_with(ctx, part):
    cases.case_tampered_keys(ctx, part)


def test_ptau_verify_and_pk_verify_on_the_deposit_key(ctx):
    cases.case_deposit_key(ctx)
