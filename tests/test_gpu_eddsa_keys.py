"""GPU parity: BabyJubJub compressed keys, key derivation and batched signing against oracle/py/babyjubjub.py; cases in
tests/eddsa_keys_cases.py.  The two seams exist in the hooks build only."""
import pytest

from tests import eddsa_keys_cases as kc

pytestmark = pytest.mark.gpu

SIZES, REUSE = (0, 1, 63, 64, 65, 4097), (4097, 65, 4097)


def test_fr_sqrt_seam(ctx_hooks):
    """every depth of Tonelli-Shanks once, zero, non-residues, random squares (og_hook_fr_sqrt_d)"""
    kc.case_fr_sqrt(ctx_hooks)


def test_sign_s_seam(ctx_hooks):
    """s = (r + h sk) mod ORDER at its edges, s >= r included (og_hook_ed_sign_s_d)"""
    kc.case_sign_s(ctx_hooks)


def test_decompress(ctx):
    kc.case_decompress(ctx)


def test_pubkey(ctx):
    kc.case_pubkey(ctx)


def test_sign(ctx):
    """records byte for byte, then sign -> verify and sign -> verify_compressed on the device's own output"""
    kc.case_sign(ctx)


def test_verify_compressed(ctx):
    """every pool record of tests/eddsa_cases.py with its key compressed, keys without a root, refused encodings"""
    kc.case_verify_compressed(ctx)


@pytest.mark.parametrize("name", ("decompress", "pubkey", "sign", "verify_compressed"))
def test_shapes(ctx, name):
    """one lane to 65 waves, tiled from a prime-sized pool at two offsets; then a larger call followed by a smaller one"""
    kc.case_shapes(ctx, name, SIZES, REUSE)
