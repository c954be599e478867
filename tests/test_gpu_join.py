"""The join statement on the GPU through the C ABI; cases in tests/join_cases.py."""
import numpy as np
import pytest

from tests import join_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases._key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 70), (32, 3 + 2)])
def test_join_r1cs_and_witness_match_spec(ctx, depth, n):
    """depth 2 with 70 requests: 140 lanes, past two waves with a ragged tail (a pair never straddles a wave, the last wave is
    partial); depth 32: the deployed tree, the five edge requests (three would leave two of them out)"""
    cases.case_r1cs_and_witness_match_spec(ctx, depth, n=n)


def test_join_end_to_end_depth2(ctx):
    cases.case_join_end_to_end(ctx, 2, n=4)


def test_join_end_to_end_depth32(ctx, key32):
    cases.case_join_end_to_end(ctx, 32, n=2, key=key32)


def test_join_forgeries_are_unprovable(ctx):
    cases.case_forgeries_are_unprovable(ctx, 2)


def test_join_different_roots(ctx):
    cases.case_different_roots(ctx, 2)


def test_join_record_boundary(ctx):
    cases.case_record_boundary(ctx, 2)


def _le(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32)


def test_join_batch_1027_verifies_and_matches_the_c_restatement(ctx, key32):
    """a throughput-shaped call: 1 027 depth-32 requests in one og_join_prove_batch_d (more than one sub-batch, a ragged last one),
    every pair of notes meeting at level 0 (each note's first sibling is the other's leaf, computed with og_mimc7_hash2_d; the 31
    siblings above are shared), all accepted by og_verify_batch_d under an og_vk_load of the key with n_pub = 5, proof 0 against
    proof 1's inputs refused, proofs 0, 63, 64 and 1 026 -- four of the edge requests -- byte-identical to the C restatement"""
    import random
    from oracle.c import binding as oc
    from owshen_amd import circuit, groth16 as g16
    depth, n = 32, 1027
    blob, vk, pk, _close = key32
    rnd = random.Random(1027)
    rng = np.random.default_rng(1027)
    recs = rng.integers(0, 256, (n, 11 + 2 * depth, 32), dtype=np.uint8)
    recs[:, :, 31] &= 0x1F                       # every field < 2^253 < r
    recs[:, (2, 6), 15:] = 0                     # amount_a, amount_b < 2^120
    recs[:, (3, 7), 4:] = 0                      # indices < 2^32 ...
    recs[:, 3, 0] &= 0xFE                        # ... a left child and
    recs[:, 7, 0] |= 0x01                        # a right child at level 0,
    recs[:, 7, 1:] = recs[:, 3, 1:]              # under one parent
    recs[:, 7, 0] = recs[:, 3, 0] | 0x01
    recs[:, 11 + depth + 1:] = recs[:, 11 + 1:11 + depth]        # the siblings above level 0 are shared

    def h2(l, r):
        return ctx.to_host(ctx.mimc7_hash2(ctx.to_device(np.ascontiguousarray(l)), ctx.to_device(np.ascontiguousarray(r))))

    leaf = [h2(h2(recs[:, o], recs[:, o + 1]), h2(recs[:, o + 2], recs[:, 8])) for o in (0, 4)]
    recs[:, 11] = leaf[1]                        # sibling a of level 0 = leaf b
    recs[:, 11 + depth] = leaf[0]                # sibling b of level 0 = leaf a
    edge = cases.edge_inputs(rnd, depth, 5)
    for k, t in enumerate((0, 63, 64, 1026)):
        recs[t] = cases._pack(circuit, edge[k])
    rs = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rs[:, 31] &= 0x1F
    rs[:, 63] &= 0x1F
    recs_d = ctx.to_device(recs)
    proofs, pub = circuit.join_prove(ctx, pk, depth, recs_d, rs, return_public=True)
    assert pub[:, 3].tobytes() == recs[:, 9].tobytes()          # chain_id
    with g16.VerifyingKey(ctx, g16.vk_to_bytes(vk)) as dvk:
        assert dvk.n_pub == 5
        ok = dvk.verify_batch(pub, proofs)
        assert ok.all(), f"{int((~ok).sum())} of {n} join proofs refused"
        assert not dvk.verify_batch(pub[1:2], proofs[0:1])[0]
    idx = [0, 63, 64, 1026]
    wit = ctx.to_host(circuit.join_witness(ctx, depth, recs_d[idx]))
    ck = oc.prepared_key_from_blob(blob)
    for j, t in enumerate(idx):
        r_, s_ = int.from_bytes(rs[t][:32].tobytes(), "little"), int.from_bytes(rs[t][32:].tobytes(), "little")
        assert proofs[t].tobytes() == ck.prove(wit[j], r_, s_), t
