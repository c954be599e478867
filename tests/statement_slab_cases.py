"""The slab loop every statement's records -> proofs call shares (groth16.hip, statement_prove_batch), past its first slab: cases for
the CPU-interpreter run and the GPU run.

A slab is 65 535 records unless the circuit is enormous, so no other test reaches a second one: the offsets into the records, the
blinding pairs, the proofs and the public outputs, and the record index in the two messages, only ever ran with a first record of 0.
OG_SLAB_MAX (hooks builds) bounds the slab: 5 requests with a bound of 2 are three slabs, the last one ragged.  Per statement
(depth 2; withdraw without padding and with OG_GEN_ONE_SUB=0, so that it takes the slab loop and not its in-pipeline generator):
  - without the hook: the public outputs are the witnesses' wires, proofs 0, 2 and 4 are the C restatement's bytes and og_verify
    accepts them (what the statement's end-to-end case expects of the call);
  - with the hook: three witness launches where the unhooked call makes one (the profiler's count: the hook is honoured), and proofs
    and public outputs byte-identical to those;
  - record 3 malformed (field 0 = r): OG_ERR_INVALID naming "input record 3";
  - record 4's witness unsatisfiable: OG_ERR_UNSATISFIED naming "witness 4".  Only join has records that pass the boundary check and
    give such a witness (two notes under different roots, join_cases.case_different_roots); a forged witness, the way
    case_overdraw_is_unprovable and the forgeries of join and transfer go, enters through og_prove_batch_d and never meets the loop."""
import contextlib
import os
import random

import numpy as np
import pytest

from oracle.py import fields

R = fields.R
DEPTH = 2
N = 5
STATEMENTS = ("withdraw", "deposit", "split", "join", "transfer")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _statement(ctx, st, rnd):
    """(key blob, vk, key, close, records [N], prove(recs_d, rs, return_public), witness(recs_d), hooks of every call, a record whose
    witness is unsatisfiable | None)"""
    from owshen_amd import circuit
    from tests import deposit_cases, join_cases, split_cases, transfer_cases, withdraw_cases
    env, unsat = {}, None
    if st == "withdraw":
        _r1, blob, vk, pk, close = withdraw_cases._key(ctx, DEPTH, 0, 0)
        recs = [withdraw_cases._pack(circuit, withdraw_cases._inputs(rnd, DEPTH)) for _ in range(N)]
        prove = lambda d, rs, pub=False: circuit.prove_from_inputs(ctx, pk, DEPTH, d, rs, return_public=pub)
        witness = lambda d: circuit.witness(ctx, DEPTH, d)
        env = {"OG_GEN_ONE_SUB": "0"}
    elif st == "deposit":
        from owshen_amd import groth16 as g16
        blob, vk = g16.setup(ctx, circuit.deposit_r1cs(ctx.mimc7_constants()), 41, 42, 43, 44, 45)
        pk = g16.ProvingKey(ctx, blob)
        close = pk.close
        recs = [circuit.pack_deposit_inputs(rnd.randrange(R), rnd.randrange(R), rnd.randrange(1 << 160)) for _ in range(N)]
        prove = lambda d, rs, pub=False: circuit.deposit_prove(ctx, pk, d, rs, return_public=pub)
        witness = lambda d: circuit.deposit_witness(ctx, d)
    else:
        cases = {"split": split_cases, "join": join_cases, "transfer": transfer_cases}[st]
        blob, vk, pk, close = cases._key(ctx, DEPTH)
        ins = cases.edge_inputs(rnd, DEPTH, N)
        recs = [cases._pack(circuit, i) for i in ins]
        prove = lambda d, rs, pub=False: getattr(circuit, st + "_prove")(ctx, pk, DEPTH, d, rs, return_public=pub)
        witness = lambda d: getattr(circuit, st + "_witness")(ctx, DEPTH, d)
        if st == "join":   # note b under another root: the boundary check cannot see it, the prover's row check does
            i = ins[4]
            unsat = cases._pack(circuit, dict(i, siblings_b=i["siblings_b"][:-1] + [(i["siblings_b"][-1] + 1) % R]))
    return blob, vk, pk, close, np.stack(recs), prove, witness, env, unsat


def case_second_slab(ctx, st):
    from oracle.c import binding as oc
    from owshen_amd import api, groth16 as g16
    rnd = random.Random(STATEMENTS.index(st) + 600)
    blob, vk, pk, close, recs, prove, witness, env, unsat = _statement(ctx, st, rnd)
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(N)]
    with _env(**env):
        assert "OG_SLAB_MAX" not in os.environ
        proofs, pub = prove(ctx.to_device(recs), rs, True)
        wit = ctx.to_host(witness(ctx.to_device(recs)))
        n_pub = pub.shape[1]
        assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:1 + n_pub]).tobytes()
        ck, vkb = oc.prepared_key_from_blob(blob), g16.vk_to_bytes(vk)
        for t in (0, 2, 4):
            assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"{st} proof {t} differs from the C restatement"
            assert g16.verify(vkb, api.bytes_to_ints(pub[t]), proofs[t].tobytes(), lib=ctx._lib) is True
        def witness_calls(call):
            """what `call` returns, and how many witness launches it made (one profiled region per slab)"""
            ctx.profile(True)
            try:
                out = call()
                return out, ctx.profile_read()["witness"][1]
            finally:
                ctx.profile(False)

        _, slabs = witness_calls(lambda: prove(ctx.to_device(recs), rs))
        assert slabs == 1, f"{st}: {slabs} slabs without the hook"
        with _env(OG_SLAB_MAX="2"):
            (p2, pub2), slabs = witness_calls(lambda: prove(ctx.to_device(recs), rs, True))
            assert slabs == 3, f"{st}: OG_SLAB_MAX=2 gave {slabs} slabs for {N} requests, not 3"
            assert p2.tobytes() == proofs.tobytes(), f"{st}: three slabs give other proofs than one"
            assert pub2.tobytes() == pub.tobytes(), f"{st}: three slabs give other public outputs than one"
            assert prove(ctx.to_device(recs), rs).tobytes() == proofs.tobytes()      # public_out = NULL
            bad = recs.copy()
            bad[3, 0] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
            with pytest.raises(api.OwshenGpuError) as e:
                prove(ctx.to_device(bad), rs)
            assert e.value.code == -1 and "input record 3: field 0 " in str(e.value), str(e.value)
            if unsat is not None:
                bad = recs.copy()
                bad[4] = unsat
                with pytest.raises(api.OwshenGpuError) as e:
                    prove(ctx.to_device(bad), rs)
                assert e.value.code == -4 and "witness 4 does not satisfy" in str(e.value), str(e.value)
    close()
