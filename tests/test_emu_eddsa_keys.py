"""Compressed keys, key derivation and batched signing on the CPU interpreter (tests/hipemu); cases in tests/eddsa_keys_cases.py."""
import pytest

from tests import eddsa_keys_cases as kc

SIZES, REUSE = (0, 1, 64, 65, 129), (129, 65, 129)


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_emu_fr_sqrt_seam(ectx):
    """every depth of Tonelli-Shanks once, zero, non-residues, random squares (og_hook_fr_sqrt_d)"""
    kc.case_fr_sqrt(ectx)


def test_emu_sign_s_seam(ectx):
    """s = (r + h sk) mod ORDER at its edges, s >= r included (og_hook_ed_sign_s_d)"""
    kc.case_sign_s(ectx)


def test_emu_decompress(ectx):
    kc.case_decompress(ectx)


def test_emu_pubkey(ectx):
    kc.case_pubkey(ectx)


def test_emu_sign(ectx):
    """records byte for byte, then sign -> verify and sign -> verify_compressed on the device's own output"""
    kc.case_sign(ectx)


def test_emu_verify_compressed(ectx):
    """the edge records of tests/eddsa_cases.py with their keys compressed, keys without a root, refused encodings"""
    kc.case_verify_compressed(ectx, 59)


@pytest.mark.parametrize("name", ("decompress", "pubkey", "sign", "verify_compressed"))
def test_emu_shapes(ectx, name):
    """up to three workgroups, tiled from a prime-sized pool at two offsets; then a larger call followed by a smaller one"""
    kc.case_shapes(ectx, name, SIZES, REUSE)
