"""The quotient in the evaluation form on the CPU interpreter (tests/hipemu); cases in tests/h_eval_cases.py.  The two circuits
of domain 32 through every schedule; keys of the larger domains run on the GPU (test_gpu_h_eval.py), and here their stage-block
shapes run through the quotient's half of the form alone (case_coset_pipeline_shapes: no key, no DFT over points)."""
import pytest

from tests import h_eval_cases as cases

CIRCUITS = ["W", "PC"]


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_fan_out(ectx, name, n):
    cases.case_fan_out(ectx, name, n)


@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_serial(ectx, name):
    cases.case_serial(ectx, name)


@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_through_the_stage_pipeline(ectx, name, monkeypatch):
    cases.case_pipeline(ectx, name, monkeypatch)


@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_window_sharded_front(ectx, name):
    cases.case_sharded(ectx, name)


@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_radix_2_kernel(ectx, name, monkeypatch):
    cases.case_radix2(ectx, name, monkeypatch)


def test_emu_h_eval_unsatisfied_witness_is_named(ectx):
    cases.case_unsatisfied(ectx)


def test_emu_h_eval_flag_1_key_keeps_the_old_form(ectx):
    cases.case_flag1_key_keeps_the_old_form(ectx)


def test_emu_h_eval_key_below_the_bound_keeps_the_old_form(ectx):
    cases.case_below_the_bound(ectx)


def test_emu_h_eval_fold_reaches_public_and_constant_wires(ectx):
    cases.case_fold_reaches_public_and_constant_wires(ectx)


def test_emu_h_eval_load_is_refused_while_a_job_is_pending(ectx):
    cases.case_load_is_refused_while_a_job_is_pending(ectx, load_after=False)


@pytest.mark.parametrize("log_d", [5, 11, 12, 13])
def test_emu_h_eval_coset_pipeline_shapes(ectx, log_d, monkeypatch):
    cases.case_coset_pipeline_shapes(ectx, log_d, monkeypatch)


@pytest.mark.parametrize("name", CIRCUITS)
def test_emu_h_eval_merged_and_unmerged_differ(ectx, name):
    cases.case_merged_and_unmerged_differ(ectx, name)


@pytest.mark.parametrize("which", ["1", "2"])
def test_emu_h_eval_corrupted_tables_are_refused(ectx, which):
    cases.case_corrupted_tables_are_refused(ectx, which)
