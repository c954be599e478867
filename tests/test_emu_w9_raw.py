"""The wave-wide field forms at their operand bounds on the CPU interpreter, through og_hook_w9_raw_d -- cases, integer models and
checks are in tests/w9_raw_cases.py; tests/test_gpu_w9_raw.py runs the same on the hardware."""
import pytest

from tests import w9_raw_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name,field", cases.PARAMS)
def test_emu_w9_raw(ectx, name, field):
    n, seen = cases.run(ectx, name, field)
    assert n == len(cases.table(name, field)) and n >= 8
