"""The quotient in the evaluation form on the GPU through the C ABI; cases in tests/h_eval_cases.py.  The form is forced at toy
size through OG_H_FORM, so every case runs the hooks build; the shipped library crosses the rule's bound by itself in the
full-size parity tests (test_gpu_fullsize_pipeline.py, test_gpu_row_form.py: domain 2^17 against the C restatement)."""
import pytest

from tests import h_eval_cases as cases

pytestmark = pytest.mark.gpu
CIRCUITS = ["W", "D11", "WD", "PC"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_fan_out(ctx_hooks, name, n):
    cases.case_fan_out(ctx_hooks, name, n)


@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_serial(ctx_hooks, name):
    cases.case_serial(ctx_hooks, name)


@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_through_the_stage_pipeline(ctx_hooks, name, monkeypatch):
    cases.case_pipeline(ctx_hooks, name, monkeypatch)


@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_window_sharded_front(ctx_hooks, name):
    cases.case_sharded(ctx_hooks, name)


@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_radix_2_kernel(ctx_hooks, name, monkeypatch):
    cases.case_radix2(ctx_hooks, name, monkeypatch)


def test_h_eval_unsatisfied_witness_is_named(ctx_hooks):
    cases.case_unsatisfied(ctx_hooks)


def test_h_eval_flag_1_key_keeps_the_old_form(ctx_hooks):
    cases.case_flag1_key_keeps_the_old_form(ctx_hooks)


def test_h_eval_key_below_the_bound_keeps_the_old_form(ctx_hooks):
    cases.case_below_the_bound(ctx_hooks)


def test_h_eval_fold_reaches_public_and_constant_wires(ctx_hooks):
    cases.case_fold_reaches_public_and_constant_wires(ctx_hooks)


def test_h_eval_load_is_refused_while_a_job_is_pending(ctx_hooks):
    cases.case_load_is_refused_while_a_job_is_pending(ctx_hooks, load_after=True)


@pytest.mark.parametrize("log_d", [5, 11, 12, 13])
def test_h_eval_coset_pipeline_shapes(ctx_hooks, log_d, monkeypatch):
    cases.case_coset_pipeline_shapes(ctx_hooks, log_d, monkeypatch)


@pytest.mark.parametrize("name", CIRCUITS)
def test_h_eval_merged_and_unmerged_differ(ctx_hooks, name):
    cases.case_merged_and_unmerged_differ(ctx_hooks, name)


@pytest.mark.parametrize("which", ["1", "2"])
def test_h_eval_corrupted_tables_are_refused(ctx_hooks, which):
    cases.case_corrupted_tables_are_refused(ctx_hooks, which)
