"""GPU: the chains of tests/ec_chain_cases.py (310 additions without normalisation from non-canonical X representatives up to
the weak invariant's bound) on the hardware, one launch per group through og_hook_ec_chain_d of the hooks build."""
import pytest

from tests import ec_chain_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", [1, 2])
def test_gpu_ec_chain(ctx_hooks, group):
    assert cases.run(ctx_hooks, group) == 2 * 6 * (len(cases.CUTS) + 1)
