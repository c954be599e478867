"""GPU: the Fr-side kernels between the transforms and the multi-scalar multiplications, each against integers of its own; cases
in tests/fr_side_cases.py.  The Lagrange basis, the sparse row product and og_setup's refusals run the shipped library; the
quotient's evaluation form (OG_H_POLY_COSET) and the boundary key in that form (OG_H_FORM) need the hooks build.

Host time: the expected coset values are the C restatement's (two transforms per distinct input row, each row once per session)
and a product of Python integers.  On the MI355X host the 65 cases of this file took 5.0 s together, expected values included:
0.68 s for the four extreme triples at 2^17 (radix-4 and radix-2 kernel, batches of two), 0.44 s for the block-shape inputs at
2^17, 0.3 s for the boundary key's setup and loads, under 0.1 s for every other case -- all below the 1.0 s of the slowest
extreme-input case in test_gpu_quotient_shapes.py, so no size was taken off the list.

What these cases do NOT pin: with nt_reduce_64n taken out of the pw_mul branch of k_ntt_block4 (tried on the interpreter build)
every coset case still passes.  The reduction is not needed for a right answer: v < 36N and pw_a < 4N (the other transform stores
its values through nt_reduce_64n), so the product's operands stay within fe_mul's own bound, 36N x 4N = 144 N^2 < 169 N^2 =
N 2^261, and the result is below 2N either way."""
import pytest

from tests import fr_side_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.LAG_TAUS)
@pytest.mark.parametrize("log_d", cases.LAG_SIZES)
def test_lagrange_basis(ctx, log_d, name):
    cases.case_lagrange(ctx, log_d, name)


@pytest.mark.parametrize("name", list(cases.LAG_BAD_TAUS))
def test_lagrange_refuses_a_non_canonical_tau(ctx, name):
    cases.case_lagrange_refuses(ctx, name)


@pytest.mark.parametrize("n_rows", cases.SPMV_ROWS)
def test_spmv_against_integers(ctx, n_rows):
    cases.case_spmv(ctx, n_rows)


def test_boundary_key_runs_a_and_b_over_the_rows(ctx):
    cases.case_boundary_forms(ctx)


def test_boundary_proofs_are_the_plain_blobs_and_the_oracles(ctx):
    cases.case_boundary_proofs(ctx)


@pytest.mark.parametrize("which", [0, 1])
def test_boundary_unsatisfied_tail_entry_is_named(ctx, which):
    cases.case_boundary_unsatisfied(ctx, which)


def test_boundary_key_in_the_evaluation_form(ctx_hooks):
    cases.case_boundary_eval_form(ctx_hooks)


@pytest.mark.parametrize("log_d", [4, 10, 11, 14, 17])
def test_coset_quotient_on_extreme_inputs(ctx_hooks, log_d):
    cases.case_coset_extremes(ctx_hooks, log_d)


@pytest.mark.parametrize("log_d", [10, 14, 17])
def test_coset_quotient_block_shapes(ctx_hooks, log_d):
    cases.case_coset_block_shapes(ctx_hooks, log_d)


def test_setup_refuses_bad_toxic_values(ctx):
    cases.case_setup_refusals(ctx)
