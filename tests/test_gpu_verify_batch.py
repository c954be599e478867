"""og_vk_load / og_verify_batch_d on the GPU: the cases of tests/verify_batch_cases.py at full size, then batches at size --
1024 deposit proofs and 64 natural depth-32 withdraw proofs from the product's own prover, every eighth corrupted in a rotating
class, one call each, against og_verify over every proof through a 16-thread pool."""
import random

import numpy as np
import pytest

from oracle.py import fields
from tests import verify_batch_cases as cases

pytestmark = pytest.mark.gpu


def test_mixed_batch_decides_as_og_verify(ctx):
    cases.case_mixed_batch(ctx, small=False)


def test_vkx_at_infinity_skips_gammas_pairing(ctx):
    cases.case_vkx_infinity_accept(ctx)


def test_published_eip197_vector(ctx):
    cases.case_eip197_vector(ctx)


def test_key_handling(ctx):
    cases.case_keys(ctx)


def test_final_exponentiation_chain_decides_as_the_plain_power(ctx_hooks):
    cases.case_final_exponentiation_pin(ctx_hooks)


def _corrupt_every_eighth(proofs, pub, rnd):
    """in place: entry 8k gets class k mod 6"""
    n = proofs.shape[0]
    p_le = np.frombuffer(fields.P.to_bytes(32, "little"), dtype=np.uint8)
    for k, i in enumerate(range(0, n, 8)):
        c = k % 6
        if c == 0:
            proofs[i, rnd.randrange(64)] ^= 1 << rnd.randrange(8)            # a bit of A
        elif c == 1:
            proofs[i, 64 + rnd.randrange(128)] ^= 1 << rnd.randrange(8)      # a bit of B
        elif c == 2:
            proofs[i, 192 + rnd.randrange(64)] ^= 1 << rnd.randrange(8)      # a bit of C
        elif c == 3:
            proofs[i, 192:256] = 0                                           # C = infinity
        elif c == 4:
            pub[i] = pub[(i + 1) % n]                                        # a neighbour's statement
        else:
            v = int.from_bytes(proofs[i, 0:32].tobytes(), "little") + fields.P
            proofs[i, 0:32] = np.frombuffer((v % (1 << 256)).to_bytes(32, "little"), dtype=np.uint8)   # A.x + p
    return proofs, pub


def _check_at_size(ctx, vkb, proofs, pub):
    from owshen_amd import api, groth16 as g16
    n = proofs.shape[0]
    entries = [(api.bytes_to_ints(pub[i]), proofs[i].tobytes()) for i in range(n)]
    want = cases.expected(vkb, entries, threads=16)
    with g16.VerifyingKey(ctx, vkb) as key:
        proofs_d, pub_d = ctx.to_device(proofs), ctx.to_device(pub)
        got = key.verify_batch(pub_d, proofs_d)
        again = key.verify_batch(pub_d, proofs_d)
    assert got.tolist() == want.tolist(), np.nonzero(got != want)[0][:16]
    assert again.tolist() == got.tolist()
    bad = np.zeros(n, dtype=bool)
    bad[::8] = True
    assert not want[bad].any() and want[~bad].all()


def test_1024_deposit_proofs_in_one_call(ctx):
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(1024)
    r1 = circuit.deposit_r1cs(ctx.mimc7_constants())
    blob, vk = g16.setup(ctx, r1, 41, 42, 43, 44, 45)
    pk = g16.ProvingKey(ctx, blob)
    n = 1024
    recs = np.stack([circuit.pack_deposit_inputs(rnd.randrange(fields.R), rnd.randrange(fields.R), rnd.randrange(1 << 160)) for _ in range(n)])
    rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in range(n)]
    proofs, pub = circuit.deposit_prove(ctx, pk, ctx.to_device(recs), rs, return_public=True)
    pk.close()
    proofs, pub = _corrupt_every_eighth(proofs.copy(), pub.copy(), rnd)
    _check_at_size(ctx, g16.vk_to_bytes(vk), proofs, pub)


def test_64_natural_withdraw_proofs_in_one_call(ctx):
    from owshen_amd import circuit, groth16 as g16
    from tests.withdraw_cases import _inputs, _key, _pack
    rnd = random.Random(64)
    depth = 32
    _r1, _blob, vk, pk, close = _key(ctx, depth, 0, 0)
    n = 64
    packed = np.stack([_pack(circuit, _inputs(rnd, depth)) for _ in range(n)])
    rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in range(n)]
    proofs, pub = circuit.prove_from_inputs(ctx, pk, depth, ctx.to_device(packed), rs, return_public=True)
    close()
    proofs, pub = _corrupt_every_eighth(proofs.copy(), pub.copy(), rnd)
    _check_at_size(ctx, g16.vk_to_bytes(vk), proofs, pub)
