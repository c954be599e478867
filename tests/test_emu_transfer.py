"""The transfer statement on the CPU interpreter (tests/hipemu); cases in tests/transfer_cases.py.  Where the walk's form is not what a
case is about it takes the lane-local kernel: every cross-lane read of the wave-wide walk is a rendezvous of the whole workgroup on
the interpreter."""
import random

import pytest

from tests import transfer_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("depth,env", [(1, cases.LANE_LOCAL), (2, {})])
def test_emu_transfer_r1cs_and_witness_match_spec(ectx, depth, env):
    """depth 1 through k_transfer_core, depth 2 through the walk a call of five requests takes by default: k_tw9_*"""
    with cases.walk(**env):
        cases.case_r1cs_and_witness_match_spec(ectx, depth, n=5)


@pytest.mark.parametrize("n", [1, 3])
def test_emu_transfer_walks_agree(ectx, n):
    rnd = random.Random(40 + n)
    cases.case_walks_agree(ectx, 2, cases.edge_inputs(rnd, 2, 5)[:n])


def test_emu_transfer_end_to_end(ectx):
    with cases.walk(**cases.LANE_LOCAL):
        cases.case_transfer_end_to_end(ectx, 2, n=2)


def test_emu_transfer_forgeries_are_unprovable(ectx):
    cases.case_forgeries_are_unprovable(ectx, 2)


def test_emu_transfer_record_boundary(ectx):
    with cases.walk(**cases.LANE_LOCAL):
        cases.case_record_boundary(ectx, 2)


def test_emu_transfer_notes_are_spendable(ectx):
    with cases.walk(**cases.LANE_LOCAL):
        cases.case_notes_are_spendable(ectx, 4)
