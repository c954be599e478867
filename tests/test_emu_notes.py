"""Stealth notes on the CPU interpreter (tests/hipemu): sealing, scanning, the uniform-scalar seam and a note through the pool; cases
in tests/note_cases.py, the scheme in tests/note_spec.py."""
import pytest

from tests import note_cases as nc

SIZES, REUSE = (0, 1, 64, 65, 129), (129, 65)


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_emu_mul_uniform_seam(ectx):
    """s P for one scalar over all lanes = multiply(P, s): the recoding's edges over BASE, the identity, the eight small points, a
    mixed-order point and random points (og_hook_ed_mul_uniform_d)"""
    nc.case_mul_uniform(ectx)


def test_emu_seal(ectx):
    """memos and notes byte for byte, every refusal on its own"""
    nc.case_seal(ectx)


def test_emu_scan(ectx):
    """every class of memo under four scanning keys, with and without leaves, with and without the opened rows"""
    nc.case_scan(ectx)


def test_emu_scan_refuses_a_non_canonical_sk(ectx):
    nc.case_scan_refuses_a_non_canonical_sk(ectx)


@pytest.mark.parametrize("name", ("seal", "scan"))
def test_emu_shapes(ectx, name):
    """up to three workgroups, tiled from a prime-sized pool at two offsets; then a larger call followed by a smaller one"""
    nc.case_shapes(ectx, name, SIZES, REUSE)


def test_emu_through_the_pool(ectx):
    """seal -> transfer (pay_leaf = the sealed leaf) -> append -> scan -> withdraw the opened note -> og_verify, depth 2"""
    nc.case_through_the_pool(ectx)
