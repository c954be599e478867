"""og_ptau_verify / og_pk_verify on the CPU interpreter (tests/hipemu); cases in tests/ptau_verify_cases.py.  Stops at power 5."""
import pytest

from tests import ptau_cases, ptau_verify_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("power", [1, 2, 5])
def test_emu_ptau_verify_accepts_a_ceremony(ectx, power):
    cases.case_valid_file(ectx, power)


@pytest.mark.parametrize("power,names", [(1, cases.ALL_TAMPERED), (2, cases.ALL_TAMPERED[:6]), (2, cases.ALL_TAMPERED[6:]), (5, cases.SIZE_TAMPERED)])
def test_emu_ptau_verify_names_what_was_tampered_with(ectx, power, names):
    cases.case_tampered_files(ectx, power, names)


def test_emu_ptau_verify_refusals(ectx):
    cases.case_file_refusals(ectx)
    cases.case_null_handles(ectx._lib)


def test_emu_verify_calls_are_refused_while_a_job_is_pending(ectx, monkeypatch):
    """(the switches of test_emu_withdraw.py's job tests: a toy call goes through the stage pipeline and really stays enqueued)"""
    monkeypatch.setenv("OG_SUB_BATCH", "2")
    monkeypatch.setenv("OG_PIPE_MIN", "1")
    monkeypatch.setenv("OG_GEN_MIN", "1")
    cases.case_refused_while_a_job_is_pending(ectx)


@pytest.mark.parametrize("extra_power", [0, 2])
def test_emu_pk_verify_accepts_the_keys_of_the_file(ectx, extra_power):
    cases.case_valid_keys(ectx, ptau_cases._small(25, 3), 125, extra_power)


def test_emu_pk_verify_accepts_an_exported_and_imported_key(ectx):
    cases.case_exported_and_imported_key(ectx)


def test_emu_pk_verify_foreign_keys(ectx):
    cases.case_foreign_keys(ectx)


@pytest.mark.parametrize("part", [0, 1, 2])
def test_emu_pk_verify_names_what_was_tampered_with(ectx, part):
    cases.case_tampered_keys(ectx, part)


def test_emu_verify_command_line(ectx, tmp_path, capsys):
    cases.case_cli(ectx, tmp_path, capsys)
