"""GPU: the routines of the single-Q addition ALONE on the hardware -- the SQR_PLUS / SQR_ADD_PLUS asm statements and the
limb-wise helpers and Fq2 forms around them -- on the raw-limb cases of tests/field_rider_cases.py, limb for limb against Python
integers.  One launch per parameter through og_hook_fe_raw_d of the hooks build."""
import pytest

from tests import field_raw_cases as frc
from tests import field_rider_cases as rider

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,field", rider.PARAMS)
def test_gpu_field_rider(ctx_hooks, name, field):
    frc.run(ctx_hooks, name, field)
