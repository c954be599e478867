"""The Fr-side kernels on the CPU interpreter (tests/hipemu); cases in tests/fr_side_cases.py.  The quotient's evaluation form
runs its extreme inputs at 2^4, 2^10 and 2^11 here and the block-shape inputs at 2^10 and 2^14; the extreme inputs at 2^14 and
everything at 2^17 run on the GPU (test_gpu_fr_side.py).  The boundary key loads in the evaluation form here too: domain 16, the
whole case takes 3.5 s, less than any key of test_emu_h_eval.py."""
import pytest

from tests import fr_side_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", cases.LAG_TAUS)
@pytest.mark.parametrize("log_d", cases.LAG_SIZES)
def test_emu_lagrange_basis(ectx, log_d, name):
    cases.case_lagrange(ectx, log_d, name)


@pytest.mark.parametrize("name", list(cases.LAG_BAD_TAUS))
def test_emu_lagrange_refuses_a_non_canonical_tau(ectx, name):
    cases.case_lagrange_refuses(ectx, name)


@pytest.mark.parametrize("n_rows", cases.SPMV_ROWS)
def test_emu_spmv_against_integers(ectx, n_rows):
    cases.case_spmv(ectx, n_rows)


def test_emu_boundary_key_runs_a_and_b_over_the_rows(ectx):
    cases.case_boundary_forms(ectx)


def test_emu_boundary_proofs_are_the_plain_blobs_and_the_oracles(ectx):
    cases.case_boundary_proofs(ectx)


@pytest.mark.parametrize("which", [0, 1])
def test_emu_boundary_unsatisfied_tail_entry_is_named(ectx, which):
    cases.case_boundary_unsatisfied(ectx, which)


def test_emu_boundary_key_in_the_evaluation_form(ectx):
    cases.case_boundary_eval_form(ectx)


@pytest.mark.parametrize("log_d", [4, 10, 11])
def test_emu_coset_quotient_on_extreme_inputs(ectx, log_d):
    cases.case_coset_extremes(ectx, log_d)


@pytest.mark.parametrize("log_d", [10, 14])
def test_emu_coset_quotient_block_shapes(ectx, log_d):
    cases.case_coset_block_shapes(ectx, log_d)


def test_emu_setup_refuses_bad_toxic_values(ectx):
    cases.case_setup_refusals(ectx)
