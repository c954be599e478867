"""The two walks of the split and the join statement on the GPU through the C ABI; cases in tests/walk_cases.py.  The shipped library
(`ctx`) takes the wave-wide walk (k_sw9_*, k_jw9_*) for calls of at most 512 requests and the lane-local kernel above; the hooks
build (`ctx_hooks`) forces either."""
import random

import numpy as np
import pytest

from tests import walk_cases as cases

pytestmark = pytest.mark.gpu

STATEMENTS = ["split", "join"]


@pytest.fixture(scope="module", params=STATEMENTS)
def key32(request, ctx):
    """one depth-32 key per statement for the module: (statement, (blob, vk, loaded key))"""
    blob, vk, pk, close = cases.STATEMENTS[request.param]._key(ctx, 32)
    yield request.param, (blob, vk, pk)
    close()


@pytest.mark.parametrize("depth,n", [(1, 1), (2, 1), (2, 3), (2, 70), (32, None)])
@pytest.mark.parametrize("statement", STATEMENTS)
def test_walks_agree(ctx_hooks, statement, depth, n):
    """depth 1: the only level is the last; 70 requests: the lane-local kernel past one wave with a ragged last one (join: 140 lanes)
    and 70 x (5 + depth) / 70 x (7 + 2 depth) one-wave workgroups in the first launch; depth 32: the deployed tree, the statement's
    edge requests"""
    n = cases.EDGE_COUNT[statement] if n is None else n
    cases.case_walks_agree(ctx_hooks, statement, depth, cases.edge_requests(statement, random.Random(80 + n), depth, n))


@pytest.mark.parametrize("depth", [1, 2])
def test_join_paths_do_not_meet_on_the_wave_wide_walk(ctx_hooks, depth):
    cases.case_join_paths_do_not_meet(ctx_hooks, depth)


def _random_records(statement, depth, n, seed):
    """n well-formed records drawn as bytes (no Python spec over a thousand requests); join's two paths need not meet: the witness
    call does not ask"""
    rng = np.random.default_rng(seed)
    if statement == "split":
        recs = rng.integers(0, 256, (n, 9 + depth, 32), dtype=np.uint8)
        recs[:, :, 31] &= 0x1F                       # every field < 2^253 < r
        recs[:, 2, 16:] = 0                          # amount < 2^128
        recs[:, 4, 15:] = 0                          # amount_out < 2^120
        recs[:, 2, 15] |= 1                          # ... < 2^120 <= amount
        recs[:, 5, 1:] = 0
        recs[:, 5, 0] &= (1 << depth) - 1            # index < 2^depth
    else:
        recs = rng.integers(0, 256, (n, 11 + 2 * depth, 32), dtype=np.uint8)
        recs[:, :, 31] &= 0x1F
        recs[:, (2, 6), 15:] = 0                     # amount_a, amount_b < 2^120: the sum is below 2^128
        recs[:, (3, 7), 1:] = 0
        recs[:, (3, 7), 0] &= (1 << depth) - 1       # both indices < 2^depth
    return recs


@pytest.mark.parametrize("n", [512, 513])
@pytest.mark.parametrize("statement", STATEMENTS)
def test_default_bound_gives_the_lane_local_bytes(ctx, ctx_hooks, statement, n):
    """the SHIPPED library at its own bound: a call of 512 requests (the wave-wide walk) and one of 513 (the lane-local kernel) return
    what the hooks build's lane-local walk returns for the same records"""
    from owshen_amd import circuit
    depth = 2
    recs = _random_records(statement, depth, n, seed=n)
    with cases.walk(**cases.LANE_LOCAL):
        want = ctx_hooks.to_host(cases.witness(circuit, statement)(ctx_hooks, depth, ctx_hooks.to_device(recs)))
    with cases.walk():
        got = ctx.to_host(cases.witness(circuit, statement)(ctx, depth, ctx.to_device(recs)))
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes()


def test_one_depth32_request_proves_and_verifies(ctx, key32):
    """one request per call, the shape the call site proves: the proof is the C restatement's, byte for byte, and og_verify accepts
    it for the returned public inputs"""
    from oracle.c import binding as oc
    from oracle.py import fields
    from owshen_amd import api, circuit, groth16 as g16
    statement, (blob, vk, pk) = key32
    depth = 32
    rnd = random.Random(3200)
    ins = cases.edge_requests(statement, rnd, depth, 2)[1:]         # the all-right walk / the divergence at the top
    rec = cases.pack(statement, ins)
    rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R))]
    with cases.walk():
        proofs, pub = cases.prove(circuit, statement)(ctx, pk, depth, ctx.to_device(rec), rs, return_public=True)
    z = cases.STATEMENTS[statement]._spec(ins[0], depth)[3]
    n_pub = pub.shape[1]
    assert api.bytes_to_ints(pub[0]) == z[1:1 + n_pub]
    assert proofs[0].tobytes() == oc.prepared_key_from_blob(blob).prove(cases._wit_bytes(z)[0], *rs[0]), f"{statement} proof differs from the C restatement"
    assert g16.verify(g16.vk_to_bytes(vk), pub[0], proofs[0].tobytes(), lib=ctx._lib) is True
