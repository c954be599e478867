"""The group law at the edge of its weak-X invariant, on the CPU interpreter: chains of 310 additions with no normalisation in
between, started from non-canonical X representatives up to the 5.5N bound, through og_hook_ec_chain_d -- cases, checks and the
oracle comparison are in tests/ec_chain_cases.py."""
import pytest

from tests import ec_chain_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("group", [1, 2])
def test_emu_ec_chain(ectx, group):
    assert cases.run(ectx, group) == 2 * 6 * (len(cases.CUTS) + 1)


def test_every_admissible_representative_starts_a_chain():
    for gid in (1, 2):
        accs, steps, expect, W = cases.build(gid)
        nf = W // 9
        js = set()
        for a, e in zip(accs, expect):
            xs = [cases.value(a[f * 9:f * 9 + 9]) for f in range(nf)]
            assert all(2 * x < 11 * cases.P for x in xs)
            assert all(x // cases.P == e[3] for x in xs)
            js.add(e[3])
            if e[3] == 5:      # "just under the bound": within 2 % of N
                assert max(xs) > 5.48 * cases.P
        assert js == set(range(6))
        assert steps.shape[1] >= 300
