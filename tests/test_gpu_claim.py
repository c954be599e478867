"""The claim statement on the GPU through the C ABI; cases in tests/claim_cases.py.  Shapes: depth 2 and the deployed depth 32; calls
of 1, 65 (past one wave, a ragged second one) and 130 requests; one depth-32 key serves the module."""
import pytest

from tests import claim_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def key32(ctx):
    """one depth-32 key for the module: (blob, vk, loaded key, close) with a `close` that does nothing"""
    blob, vk, pk, close = cases._key(ctx, 32)
    yield blob, vk, pk, (lambda: None)
    close()


@pytest.mark.parametrize("depth,n", [(2, 5), (2, 65), (2, 130), (32, 5), (32, 65)])
def test_claim_r1cs_and_witness_match_spec(ctx, depth, n):
    cases.case_r1cs_and_witness_match_spec(ctx, depth, n=n)


@pytest.mark.parametrize("n", [1, 4])
def test_claim_end_to_end_depth2(ctx, n):
    cases.case_claim_end_to_end(ctx, 2, n=n)


def test_claim_end_to_end_depth32(ctx, key32):
    cases.case_claim_end_to_end(ctx, 32, n=2, key=key32)


def test_claim_batch_130_verifies_depth32(ctx, key32):
    """130 depth-32 requests in one og_claim_prove_batch_d: all accepted by og_verify_batch_d under an og_vk_load of the key, proof 0
    against proof 1's inputs refused, proofs 0, 64 and 129 byte-identical to the C restatement"""
    import random
    import numpy as np
    from oracle.c import binding as oc
    from owshen_amd import circuit, groth16 as g16
    depth, n = 32, 130
    blob, vk, pk, _close = key32
    rnd = random.Random(130)
    ins = cases.edge_inputs(rnd, depth, n)
    recs = np.stack([cases._pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(cases.R), rnd.randrange(cases.R)) for _ in ins]
    recs_d = ctx.to_device(recs)
    proofs, pub = circuit.claim_prove(ctx, pk, depth, recs_d, rs, return_public=True)
    with g16.VerifyingKey(ctx, g16.vk_to_bytes(vk)) as dvk:
        assert dvk.n_pub == 4
        ok = dvk.verify_batch(pub, proofs)
        assert ok.all(), f"{int((~ok).sum())} of {n} claim proofs refused"
        assert not dvk.verify_batch(pub[1:2], proofs[0:1])[0]
    idx = [0, 64, 129]
    wit = ctx.to_host(circuit.claim_witness(ctx, depth, recs_d[idx]))
    ck = oc.prepared_key_from_blob(blob)
    for j, t in enumerate(idx):
        assert proofs[t].tobytes() == ck.prove(wit[j], *rs[t]), t


def test_claim_forgeries_are_unprovable(ctx):
    cases.case_forgeries_are_unprovable(ctx, 2)


def test_claim_forgeries_are_unprovable_depth32(ctx, key32):
    cases.case_forgeries_are_unprovable(ctx, 32, key=key32)


def test_claim_the_theft_is_closed(ctx):
    cases.case_the_theft_is_closed(ctx, 2)


def test_claim_record_boundary(ctx):
    cases.case_record_boundary(ctx, 2)


def test_claim_second_slab(ctx_hooks):
    cases.case_second_slab(ctx_hooks, 2)


def test_claim_through_the_pool(ctx):
    cases.case_through_the_pool(ctx, 2)
