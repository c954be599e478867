"""GPU: the wave-wide field forms (field_w9.hip.h, the w9 MiMC7 round and hash of mimc7.hip.h) at their documented operand bounds on
the hardware -- DPP row moves, v_permlane16_swap and the inline v_and_b32_dpp, which the CPU interpreter replaces by rendezvous.  One
launch per parameter through og_hook_w9_raw_d of the hooks build; cases, integer models and checks are in tests/w9_raw_cases.py."""
import pytest

from tests import w9_raw_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,field", cases.PARAMS)
def test_gpu_w9_raw(ctx_hooks, name, field):
    n, seen = cases.run(ctx_hooks, name, field)
    print(f"w9_raw {name} {cases.FIELD_NAMES[field]}: {n} cases, seen {seen}")
    assert n == len(cases.table(name, field)) and n >= 8
