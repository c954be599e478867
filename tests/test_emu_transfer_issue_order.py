"""The STRUCTURE of the transfer statement's witness call, from the interpreter's issue log (HIPEMU_ISSUE_LOG, as
tests/test_emu_issue_order.py): the wave-wide walk is three launches of one-wave workgroups -- n (7 + depth), n 5 and n 3 of them --
so the eight permutations of the two output notes run BESIDE the dependent chain, not on it (the third launch has one chain block
per request, as withdraw's); a timing comparison cannot show that.  With OG_WITNESS_W9=0 the same call is k_transfer_core."""
import random

import numpy as np
import pytest

from tests import transfer_cases as cases

DEPTH = 2


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def _launches(ectx, n, tmp_path, monkeypatch, **env):
    """(kernel, grid, block) of every launch of one og_transfer_witness_d call of n requests"""
    from owshen_amd import circuit
    rnd = random.Random(50 + n)
    recs = ectx.to_device(np.stack([cases._pack(circuit, i) for i in cases.edge_inputs(rnd, DEPTH, 5)[:n]]))
    path = str(tmp_path / "issue.log")
    with cases.walk(**env):
        circuit.transfer_witness(ectx, DEPTH, recs)          # (unlogged: grows the scratch arena to what the call needs)
        monkeypatch.setenv("HIPEMU_ISSUE_LOG", path)
        try:
            circuit.transfer_witness(ectx, DEPTH, recs)
        finally:
            monkeypatch.delenv("HIPEMU_ISSUE_LOG")
    out = []
    with open(path) as f:
        for row in (ln.split() for ln in f):
            if row and row[0] == "L":
                out.append((row[2], tuple(int(x) for x in row[3].split(",")), int(row[4])))
    return out


@pytest.mark.parametrize("n", [1, 3])
def test_emu_transfer_wave_wide_call_is_three_launches_of_one_wave_blocks(ectx, n, tmp_path, monkeypatch):
    got = _launches(ectx, n, tmp_path, monkeypatch)
    assert [(name.split("<")[0], grid[0]) for name, grid, _b in got] == [
        ("k_check_transfer_records", 1), ("k_tw9_first", n * (7 + DEPTH)), ("k_tw9_second", n * 5), ("k_tw9_chain", n * 3),
        ("k_wires_from_limbs", got[-1][1][0])], got
    assert got[0][1][1] == n and got[-1][1][1] == n               # the record / the witness is grid.y of the first and the last launch
    assert all(block == 64 and grid[1:] == (1, 1) for _name, grid, block in got[1:4]), got


@pytest.mark.parametrize("n", [1, 3])
def test_emu_transfer_lane_local_call_launches_no_wave_wide_kernel(ectx, n, tmp_path, monkeypatch):
    got = _launches(ectx, n, tmp_path, monkeypatch, OG_WITNESS_W9=0)
    assert [name.split("<")[0] for name, _g, _b in got] == ["k_check_transfer_records", "k_transfer_core", "k_wires_from_mont"], got
    assert got[1][1:] == ((1, 1, 1), 64)
