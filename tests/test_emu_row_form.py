"""The A and B queries over the QAP rows on the CPU interpreter (tests/hipemu); cases in tests/row_form_cases.py."""
import pytest

from tests import row_form_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 5])
def test_emu_row_form_proofs_are_the_plain_blobs_and_the_oracles(ectx, n):
    cases.case_same_proofs(ectx, n)


def test_emu_row_form_through_the_stage_pipeline(ectx, monkeypatch):
    cases.case_same_proofs_pipelined(ectx, monkeypatch)


def test_emu_row_form_with_the_host_assembly(ectx):
    cases.case_host_chains(ectx)


def test_emu_rule_on_the_wide_keys(ectx):
    cases.case_rule_wide_keys(ectx)


def test_emu_rule_keeps_the_natural_withdraw_key_on_the_wires(ectx):
    cases.case_rule_natural_withdraw(ectx)


def test_emu_rule_decides_at_load_whatever_the_extension(ectx, monkeypatch):
    cases.case_rule_decides_at_load(ectx, monkeypatch)


def test_emu_edge_scalars(ectx):
    cases.case_edge_scalars(ectx)


@pytest.mark.parametrize("name", cases.BAD)
def test_emu_a_wrong_extension_is_refused(ectx, name):
    cases.case_refusal(ectx, name)


@pytest.mark.parametrize("world,n", [(2, 1), (2, 4), (3, 1), (3, 4)])
def test_emu_window_sharded_front_in_row_form(ectx, world, n):
    cases.case_sharded(ectx, world, n)
