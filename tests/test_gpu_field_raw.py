"""GPU: every routine of the 9 x 29-bit Montgomery layer (owshen_amd/csrc/field.hip.h) and of the Fq2 layer above it (ec.hip.h)
ALONE on the hardware, on raw limbs at the operand bounds the routines document -- saturated, lazy (limbs up to 2^30 / 2^31) and
weak (up to 10 N) operands that never come out of fe_to_mont -- limb for limb against Python integers.  The nine asm statements of
mont_gfx950.inc are each reached directly.  Cases and reference: tests/field_raw_cases.py (the CPU interpreter runs the same list
through the same entry point in tests/test_emu_field_raw.py).  One launch per parameter through og_hook_fe_raw_d, which exists in
the hooks build only."""
import pytest

from tests import field_raw_cases as frc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,field", frc.PARAMS)
def test_gpu_field_raw(ctx_hooks, name, field):
    frc.run(ctx_hooks, name, field)
