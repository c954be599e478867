"""The shared slab loop past its first slab, on the CPU interpreter (tests/hipemu); cases in tests/statement_slab_cases.py."""
import pytest

from tests import statement_slab_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("st", cases.STATEMENTS)
def test_emu_second_slab(ectx, monkeypatch, st):
    monkeypatch.setenv("OG_WITNESS_W9", "0")   # (the lane-local walk: the wave-wide one is ~19 x the work on this interpreter, and has its own cases)
    cases.case_second_slab(ectx, st)
