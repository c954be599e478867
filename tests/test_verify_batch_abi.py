"""og_vk_load / og_vk_free / og_vk_info / og_verify_batch_d at the C ABI without a GPU: null handles are OG_ERR_INVALID (-1)
with a message, before any device call; and the arithmetic fact the final exponentiation's chain rests on."""
import ctypes as C
from math import gcd


def test_null_arguments_are_errors_without_a_device():
    from owshen_amd import _lib
    lib = _lib.lib
    null, h = C.c_void_p(), C.c_void_p()
    buf = (C.c_uint8 * 512)()
    ok = (C.c_uint32 * 4)()
    info = (C.c_uint64 * 4)()
    assert lib.og_vk_load(null, buf, 512, C.byref(h)) == -1 and b"null og_ctx" in lib.og_last_error() and not h.value
    assert lib.og_verify_batch_d(null, null, buf, buf, 1, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_verify_batch_d(null, null, buf, buf, 0, ok) == -1          # n = 0 does not excuse a null handle
    assert lib.og_vk_info(null, info) == -1 and b"og_vk_info" in lib.og_last_error()
    assert lib.og_vk_info(null, None) == -1
    lib.og_vk_free(null)                                                      # a no-op
    # a context but no key cannot be had without a device; the key check comes right after the context check (capi.hip)
    assert b"OG_" not in lib.og_last_error()


def test_python_mirror_exists():
    from owshen_amd import groth16 as g16
    assert callable(g16.VerifyingKey.verify_batch) and callable(g16.VerifyingKey.close)
    assert hasattr(g16.VerifyingKey, "__enter__") and hasattr(g16.VerifyingKey, "__exit__")


def test_chain_multiplier_is_prime_to_r():
    """k_vfy_finalexp raises to m (p^4 - p^2 + 1) / r where og_verify raises to (p^4 - p^2 + 1) / r (after the same easy part):
    m = 2x(6x^2 + 3x + 1) and gcd(m, r) = 1 -- so "is one" is the same decision.  This checks the ARITHMETIC the source comment
    claims, on a Python transcription of the chain (tests/verify_batch_cases.py: chain_multiplier); it does not see the kernel.
    What pins the kernel's chain itself is case_final_exponentiation_pin (both exponentiations on the same Miller values)."""
    from oracle.py import fields
    from tests.verify_batch_cases import chain_multiplier
    x = fields.BN_X
    m = chain_multiplier()
    assert m == 2 * x * (6 * x * x + 3 * x + 1)
    assert gcd(m, fields.R) == 1
    assert 0 < m < fields.R
