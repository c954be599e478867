"""GPU: the wave-wide G1 group law (ec_w9.hip.h: w9_xyzz_dbl / w9_xyzz_add, what k_assemble_g1_muls_w9 walks for every call of eight
requests or fewer) at the edge of its bounds table on the hardware -- the chains of tests/w9_ec_chain_cases.py, one launch per group
through og_hook_w9_ec_chain_d of the hooks build."""
import pytest

from tests import w9_ec_chain_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", range(len(cases.GROUPS)))
def test_gpu_w9_ec_chain(ctx_hooks, group):
    assert cases.run(ctx_hooks, cases.GROUPS[group]) == 5 * (len(cases.CUTS) + 1)
