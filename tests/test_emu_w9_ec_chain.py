"""The wave-wide G1 group law at the edge of its bounds table on the CPU interpreter: the chains of tests/w9_ec_chain_cases.py (the
shape of k_assemble_g1_muls_w9's walk, started from non-canonical coordinates up to 9.3 N / 5.7 N / 1.2 N) through
og_hook_w9_ec_chain_d; tests/test_gpu_w9_ec_chain.py runs the same on the hardware."""
import pytest

from tests import w9_ec_chain_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("group", range(len(cases.GROUPS)))
def test_emu_w9_ec_chain(ectx, group):
    assert cases.run(ectx, cases.GROUPS[group]) == 5 * (len(cases.CUTS) + 1)


def test_the_chains_reach_the_bounds_table_and_the_model_stays_inside_it():
    """the starting points: every admissible representative, a quarter and more at X >= 8 N and at Y >= 4 N, one coordinate within
    0.01 N of its bound; the model's own maxima (in thousandths of N) stay below the table of ec_w9.hip.h"""
    chains = cases.build()
    cov = cases.coverage(chains)
    assert cov["n"] == 40 and 4 * cov["x_ge_8N"] >= 40 and 4 * cov["y_ge_4N"] >= 40
    assert cov["jx"] == set(range(10)) and cov["jy"] == set(range(6))
    assert cov["zz_ge_N"] >= 4 and cov["zzz_ge_N"] >= 4 and cov["pushed"] >= 10
    assert cov["x_max"] >= 9290 and cov["y_max"] >= 5690
    assert sorted(set(sum(cases.GROUPS, ()))) == list(range(40))
    seen = cases.SEEN
    table = {"X": 9300, "Y": 5700, "ZZ": 1200, "ZZZ": 1200, "U": 11400, "M": 6200, "D": 17200, "P,R": 5200}
    assert set(seen) == set(table) and all(seen[k] < table[k] for k in table), dict(seen)
    assert all(len(ch.recs) == cases.N_STEPS and ch.scal[-1] != 0 for ch in chains)
