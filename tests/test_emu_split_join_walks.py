"""The two walks of the split and the join statement on the CPU interpreter (tests/hipemu); cases in tests/walk_cases.py.  Depth 1
matters: its only level is also the last, so that level's output is wire 1 -- and for join's note b nobody's wire."""
import random

import pytest

from tests import walk_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("statement", ["split", "join"])
def test_emu_walks_agree(ectx, statement, depth):
    """split's three edge requests: the all-left walk, the all-right walk, 2^128 - 1 / r - 1 operands; join's five: divergence at level
    0 and at the top, amounts 2^128 - 1 + 0 and 0 + 0, r - 1 operands"""
    n = cases.EDGE_COUNT[statement]
    cases.case_walks_agree(ectx, statement, depth, cases.edge_requests(statement, random.Random(70 + depth), depth, n))


@pytest.mark.parametrize("depth", [1, 2])
def test_emu_join_paths_do_not_meet_on_the_wave_wide_walk(ectx, depth):
    cases.case_join_paths_do_not_meet(ectx, depth)
