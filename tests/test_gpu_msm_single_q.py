"""GPU: the bucket-accumulation kernels with the single-Q mixed addition (weak X along a bucket's chain, normalised where the
bucket is stored), through the entry points tests/test_gpu_msm.py uses, against the C oracle.

One launch per group holds, by construction of the scalars (12-bit windows: a scalar d < 2^11 is the digit d of window 0 and
nothing else):
  * a bucket of ONE entry (7) and of TWO (2): the first-entry path, then one addition from an X below 2N;
  * a bucket of 320 entries (3): a long chain with no normalisation, below the heavy threshold (OG_HEAVY = 400, hooks build);
  * the same base twice in a row (4): the doubling branch inside a chain, followed by a further addition;
  * a base followed by its negative (5: the scalar 5, then 2^12 - 5 of the same base = digit -5 and a carry): the infinity
    branch, followed by the first-entry path again;
  * a bucket of 672 entries (9): over the threshold -- k_accumulate_heavy, its addition tree and k_heavy_combine;
  * every other point with a small scalar of its own; a second vector of the batch with full-size random scalars.
The add-into launch (k_accumulate_p<..., INTO>: the H query adding to the buckets the L query left) runs in the prover: a batch of
4 proofs of the withdraw statement through the stage pipeline verifies and equals the serial path byte for byte."""
import random

import numpy as np
import pytest

from oracle.py import fields
from oracle.py.curve import G1_GEN, G2_GEN, g1_to_bytes, g2_to_bytes

pytestmark = pytest.mark.gpu

N, C_BITS = 1 << 11, 12


def _le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


@pytest.mark.parametrize("precomp", [True, False])
@pytest.mark.parametrize("group", [1, 2])
def test_bucket_shapes_in_one_launch_match_c_oracle(ctx_hooks, group, precomp, monkeypatch):
    ctx = ctx_hooks  # (OG_HEAVY: hooks build)
    from owshen_amd import api
    from oracle.c import binding as oc
    rng = np.random.default_rng(700 + group)
    ks = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    ks[:, 31] &= 0x1F
    ks[324] = ks[323]      # the same base twice in a row
    ks[327] = ks[326]      # a base, then its negative (by the scalar)
    gen = np.frombuffer(g1_to_bytes(G1_GEN) if group == 1 else g2_to_bytes(G2_GEN), dtype=np.uint8)
    pts = (oc.fixed_base_g1 if group == 1 else oc.fixed_base_g2)(gen, ks)
    sc = np.zeros((2, N, 32), dtype=np.uint8)
    small = [7, 2, 2] + [3] * 320 + [4, 4, 4] + [5, (1 << C_BITS) - 5, 5] + [9] * 672
    small += [10 + (k % 1000) for k in range(N - len(small))]
    assert len(small) == N and small.count(7) == 1 and small.count(2) == 2 and small.count(3) == 320 and small.count(9) == 672
    for i, d in enumerate(small):
        sc[0, i] = _le(d)
    sc[1] = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    sc[1, :, 31] &= 0x1F
    monkeypatch.setenv("OG_HEAVY", "400")
    bases = api.Bases(ctx, group, ctx.to_device(pts), C_BITS, precomp)
    got = bases.msm(ctx.to_device(sc))
    bases.close()
    ref = oc.msm_g1 if group == 1 else oc.msm_g2
    for g in range(2):
        assert got[g].tobytes() == ref(pts, sc[g]).tobytes(), (group, precomp, g)


def test_four_withdraw_proofs_pipeline_equals_serial_and_verifies(ctx_hooks, monkeypatch):
    ctx = ctx_hooks  # (OG_PIPE_MIN: hooks build)
    from owshen_amd import circuit, groth16
    depth, n_pad3, n_pad2 = 2, 3, 70
    r1cs = circuit.withdraw_r1cs(ctx.mimc7_constants(), depth, n_pad3, n_pad2)
    blob, vk = groth16.setup(ctx, r1cs, 101, 202, 303, 404, 505)
    pk = groth16.ProvingKey(ctx, blob)
    rnd = random.Random(4)
    ins = [dict(nullifier=rnd.randrange(fields.R), secret=rnd.randrange(fields.R), amount=7 + k, recipient=9,
                pad_seed=rnd.randrange(fields.R), index=rnd.randrange(4), siblings=[rnd.randrange(fields.R) for _ in range(depth)],
                token=rnd.randrange(1 << 160), chain_id=1387) for k in range(4)]
    wit_d = circuit.witness(ctx, depth, ctx.to_device(np.stack([circuit.pack_inputs(**i) for i in ins])), n_pad3, n_pad2)
    wit = np.asarray(ctx.to_host(wit_d))
    rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in ins]
    monkeypatch.setenv("OG_SUB_BATCH", "2")
    try:
        ctx.set_lanes(1)
        assert pk.plan(4)[0] == "serial"
        want = pk.prove_batch_device(wit_d, rs)
        ctx.set_lanes(2)
        monkeypatch.setenv("OG_PIPE_MIN", "1")
        assert pk.plan(4)[0] == "stage pipeline"
        got = pk.prove_batch_device(wit_d, rs)
    finally:
        ctx.set_lanes(2)
        pk.close()
    assert got.tobytes() == want.tobytes()
    vkb = groth16.vk_to_bytes(vk)
    for k in range(4):
        assert groth16.verify(vkb, wit[k, 1:1 + r1cs.n_pub], got[k]), k
