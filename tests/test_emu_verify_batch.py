"""Batched Groth16 verification kernels (owshen_amd/csrc/verify_gpu.hip) on the CPU interpreter: the cases of
tests/verify_batch_cases.py with a small batch of the same classes (2 keys x ~25 proofs, most of them refused before the Miller
loop).  Wall time on the build container, one core: mixed batch 3.9 s (+1.6 s building the interpreter's context), final-
exponentiation pin (36 Miller values, both powers) 5.7 s, keys (120 loads) 1.5 s, the other two under 0.3 s each; an accepted
proof costs the interpreter ~12 ms, a key load ~36 ms."""
import pytest

from tests import verify_batch_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_mixed_batch_decides_as_og_verify(ectx):
    cases.case_mixed_batch(ectx, small=True)


def test_vkx_at_infinity_skips_gammas_pairing(ectx):
    cases.case_vkx_infinity_accept(ectx)


def test_published_eip197_vector(ectx):
    cases.case_eip197_vector(ectx)


def test_key_handling(ectx):
    cases.case_keys(ectx)


def test_final_exponentiation_chain_decides_as_the_plain_power(ectx):
    cases.case_final_exponentiation_pin(ectx)
