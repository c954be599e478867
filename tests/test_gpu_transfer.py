"""The transfer statement on the GPU through the C ABI; cases in tests/transfer_cases.py.  The shipped library (`ctx`) takes the
wave-wide walk for calls of at most 512 requests and the lane-local kernel above; the hooks build (`ctx_hooks`) forces either."""
import random

import numpy as np
import pytest

from tests import transfer_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases._key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 70), (32, 5)])
def test_transfer_r1cs_and_witness_match_spec(ctx, depth, n):
    """depth 2 with 70 requests: 70 x 9 one-wave workgroups in the first launch; depth 32: the deployed tree, the five edge requests"""
    cases.case_r1cs_and_witness_match_spec(ctx, depth, n=n)


@pytest.mark.parametrize("depth,n", [(2, 1), (2, 3), (2, 70), (32, 5)])
def test_transfer_walks_agree(ctx_hooks, depth, n):
    """70 requests: k_transfer_core past one wave with a ragged last one, and 70 x 9 one-wave workgroups in k_tw9_first"""
    rnd = random.Random(40 + n)
    cases.case_walks_agree(ctx_hooks, depth, cases.edge_inputs(rnd, depth, max(n, 5))[:n])


def test_transfer_end_to_end_depth2(ctx):
    cases.case_transfer_end_to_end(ctx, 2, n=4)


def test_transfer_end_to_end_depth32(ctx, key32):
    cases.case_transfer_end_to_end(ctx, 32, n=2, key=key32)


def test_transfer_forgeries_are_unprovable(ctx):
    cases.case_forgeries_are_unprovable(ctx, 2)


def test_transfer_record_boundary(ctx):
    cases.case_record_boundary(ctx, 2)


def test_transfer_notes_are_spendable(ctx):
    cases.case_notes_are_spendable(ctx, 4)


def test_transfer_batch_1027_verifies_and_matches_the_c_restatement(ctx, key32):
    """a throughput-shaped call: 1 027 depth-32 requests in one og_transfer_prove_batch_d (past the wave-wide walk's 512: the
    lane-local kernel, more than one sub-batch, a ragged last one), all accepted by og_verify_batch_d under an og_vk_load of the key
    with n_pub = 5, proof 0 against proof 1's inputs refused, proofs 0, 63, 64 and 1 026 -- four of the edge requests --
    byte-identical to the C restatement"""
    from oracle.c import binding as oc
    from owshen_amd import circuit, groth16 as g16
    depth, n = 32, 1027
    blob, vk, pk, _close = key32
    rnd = random.Random(1027)
    rng = np.random.default_rng(1027)
    recs = rng.integers(0, 256, (n, 9 + depth, 32), dtype=np.uint8)
    recs[:, :, 31] &= 0x1F                       # every field < 2^253 < r
    recs[:, 2, 15:] = 0                          # amount < 2^120
    recs[:, 7, 14:] = 0                          # pay_amount < 2^112 ...
    recs[:, 2, 14] |= 0x01                       # ... <= amount
    recs[:, 3, 4:] = 0                           # index < 2^32
    edge = cases.edge_inputs(rnd, depth, 5)
    idx = [0, 63, 64, 1026]
    for k, t in enumerate(idx):
        recs[t] = cases._pack(circuit, edge[k])
    rs = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rs[:, 31] &= 0x1F
    rs[:, 63] &= 0x1F
    recs_d = ctx.to_device(recs)
    proofs, pub = circuit.transfer_prove(ctx, pk, depth, recs_d, rs, return_public=True)
    assert pub[:, 2].tobytes() == recs[:, 5].tobytes()          # chain_id
    with g16.VerifyingKey(ctx, g16.vk_to_bytes(vk)) as dvk:
        assert dvk.n_pub == 5
        ok = dvk.verify_batch(pub, proofs)
        assert ok.all(), f"{int((~ok).sum())} of {n} transfer proofs refused"
        assert not dvk.verify_batch(pub[1:2], proofs[0:1])[0]
    wit = ctx.to_host(circuit.transfer_witness(ctx, depth, recs_d[idx]))
    ck = oc.prepared_key_from_blob(blob)
    for j, t in enumerate(idx):
        r_, s_ = int.from_bytes(rs[t][:32].tobytes(), "little"), int.from_bytes(rs[t][32:].tobytes(), "little")
        assert proofs[t].tobytes() == ck.prove(wit[j], r_, s_), t
