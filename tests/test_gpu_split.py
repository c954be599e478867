"""The split statement on the GPU through the C ABI; cases in tests/split_cases.py."""
import numpy as np
import pytest

from tests import split_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases._key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 70), (32, 3)])
def test_split_r1cs_and_witness_match_spec(ctx, depth, n):
    """depth 2 with 70 requests: past one wave with a ragged tail; depth 32: the deployed tree"""
    cases.case_r1cs_and_witness_match_spec(ctx, depth, n=n)


def test_split_end_to_end_depth2(ctx):
    cases.case_split_end_to_end(ctx, 2, n=4)


def test_split_end_to_end_depth32(ctx, key32):
    cases.case_split_end_to_end(ctx, 32, n=2, key=key32)


def test_split_overdraw_is_unprovable(ctx):
    cases.case_overdraw_is_unprovable(ctx, 2)


def test_split_record_boundary(ctx):
    cases.case_record_boundary(ctx, 2)


def test_split_batch_1027_verifies_and_matches_the_c_restatement(ctx, key32):
    """a throughput-shaped call: 1 027 depth-32 requests in one og_split_prove_batch_d (more than one sub-batch, a ragged last
    one), all accepted by og_verify_batch_d under an og_vk_load of the key with n_pub = 7, proof 0 against proof 1's inputs
    refused, proofs 0, 63, 64 and 1 026 byte-identical to the C restatement"""
    import random
    from oracle.c import binding as oc
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    depth, n = 32, 1027
    blob, vk, pk, _close = key32
    rnd = random.Random(1027)
    rng = np.random.default_rng(1027)
    recs = rng.integers(0, 256, (n, 9 + depth, 32), dtype=np.uint8)
    recs[:, :, 31] &= 0x1F                       # every field < 2^253 < r
    recs[:, 2, 16:] = 0                          # amount < 2^128
    recs[:, 4, 15:] = 0                          # amount_out < 2^120
    recs[:, 2, 15] |= 1                          # ... < 2^120 <= amount
    recs[:, 5, 4:] = 0                           # index < 2^32
    edge = cases.edge_inputs(rnd, depth, 4)
    for k, t in enumerate((0, 63, 64, 1026)):
        recs[t] = cases._pack(circuit, edge[k])
    rs = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rs[:, 31] &= 0x1F
    rs[:, 63] &= 0x1F
    recs_d = ctx.to_device(recs)
    proofs, pub = circuit.split_prove(ctx, pk, depth, recs_d, rs, return_public=True)
    assert pub[:, 3].tobytes() == recs[:, 4].tobytes() and pub[:, 2].tobytes() == recs[:, 3].tobytes()
    with g16.VerifyingKey(ctx, g16.vk_to_bytes(vk)) as dvk:
        assert dvk.n_pub == 7
        ok = dvk.verify_batch(pub, proofs)
        assert ok.all(), f"{int((~ok).sum())} of {n} split proofs refused"
        assert not dvk.verify_batch(pub[1:2], proofs[0:1])[0]
    idx = [0, 63, 64, 1026]
    wit = ctx.to_host(circuit.split_witness(ctx, depth, recs_d[idx]))
    ck = oc.prepared_key_from_blob(blob)
    for j, t in enumerate(idx):
        r_, s_ = int.from_bytes(rs[t][:32].tobytes(), "little"), int.from_bytes(rs[t][32:].tobytes(), "little")
        assert proofs[t].tobytes() == ck.prove(wit[j], r_, s_), t
