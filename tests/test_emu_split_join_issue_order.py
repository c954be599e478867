"""The STRUCTURE of the split and the join statement's witness call, from the interpreter's issue log (HIPEMU_ISSUE_LOG, as
tests/test_emu_transfer_issue_order.py): the wave-wide walk is three launches of one-wave workgroups -- n (5 + depth), 4 n and 2 n of
them for split, n (7 + 2 depth), 7 n and 4 n for join -- so the output gadgets, and join's second note, run BESIDE the dependent
chain, not on it; a timing comparison cannot show that.  With OG_WITNESS_W9=0, and above OG_WITNESS_W9_MAX, the same call is the
lane-local kernel."""
import pytest

from tests import walk_cases as cases

DEPTH = 2
WAVE_WIDE = {"split": ("k_sw9", lambda n: (n * (5 + DEPTH), 4 * n, 2 * n)),
             "join": ("k_jw9", lambda n: (n * (7 + 2 * DEPTH), 7 * n, 4 * n))}


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("statement", ["split", "join"])
def test_emu_wave_wide_call_is_three_launches_of_one_wave_blocks(ectx, statement, n, tmp_path, monkeypatch):
    got = cases.launches(ectx, statement, DEPTH, n, tmp_path, monkeypatch)
    prefix, grids = WAVE_WIDE[statement]
    first, second, chain = grids(n)
    assert [(name.split("<")[0], grid[0]) for name, grid, _b in got] == [
        (f"k_check_{statement}_records", 1), (prefix + "_first", first), (prefix + "_second", second), (prefix + "_chain", chain),
        ("k_wires_from_limbs", got[-1][1][0])], got
    assert got[0][1][1] == n and got[-1][1][1] == n               # the record / the witness is grid.y of the first and the last launch
    assert all(block == 64 and grid[1:] == (1, 1) for _name, grid, block in got[1:4]), got


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("statement", ["split", "join"])
def test_emu_lane_local_call_launches_no_wave_wide_kernel(ectx, statement, n, tmp_path, monkeypatch):
    """forced (OG_WITNESS_W9=0) and chosen (the bound one below the call): one lane per split request, two per join request"""
    for env in (dict(OG_WITNESS_W9=0), dict(OG_WITNESS_W9_MAX=n - 1)):
        got = cases.launches(ectx, statement, DEPTH, n, tmp_path, monkeypatch, **env)
        assert [name.split("<")[0] for name, _g, _b in got] == [f"k_check_{statement}_records", f"k_{statement}_core", "k_wires_from_mont"], (env, got)
        assert got[1][1:] == ((1, 1, 1), 64), (env, got)
