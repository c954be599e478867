"""The shared slab loop past its first slab, on the GPU through the hooks build (OG_SLAB_MAX exists only there); cases in
tests/statement_slab_cases.py."""
import pytest

from tests import statement_slab_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("st", cases.STATEMENTS)
def test_second_slab(ctx_hooks, st):
    cases.case_second_slab(ctx_hooks, st)
