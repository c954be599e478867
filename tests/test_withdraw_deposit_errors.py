"""Every refusal of the withdraw and deposit entry points, byte for byte: return code and the full og_last_error() text, on the CPU
interpreter at depth 2, against tests/golden/withdraw_deposit_errors.json.

The texts are a recording (`python -m tests.test_withdraw_deposit_errors` writes them), made while withdraw and deposit still
formatted their own messages, beside tests/test_record_statement_errors.py for the other three statements.  Withdraw, at
og_withdraw_shape / _witness_d / _prove_batch_d / _prove_batch_submit_d (and the refusals of og_withdraw_prove_partials_d that need
no second rank): field 0 of record 1 set to r, each sibling set to r, an index of 1 << depth, 65536 records, depth 0 and 65, an empty
batch, a null argument wherever the entry point checks one, a key of another statement (the toy key of tests/golden/key_blob), and a
well-formed batch (OG_OK) through the witness call, the blocking prover on both of its paths and the submitted one.
The malformed records reach the prover twice: as a slab (OG_GEN_ONE_SUB=0: refused by the blocking check, before anything is proved)
and inside the pipeline (the default for a call of one sub-batch: refused when the job is waited for).  Deposit, at its three entry
points: each field set to r, 65536 records, the wrong key, the null arguments, a well-formed batch.

The entries whose name ends in BRANCH_ONLY were recorded after the statements were folded onto one table: og_withdraw_witness_d
dereferenced a null pointer there before, and refuses it since."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_GOLDEN = os.path.join(_HERE, "golden", "withdraw_deposit_errors.json")
DEPTH = 2
W_REC = 8   # fields of a withdraw record before the siblings
BRANCH_ONLY = " (no check before the statement table: undefined behaviour then)"


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def compute(ctx, branch_only=True):
    from owshen_amd import circuit, groth16 as g16
    from owshen_amd.api import FR_MODULUS as R
    from tests import withdraw_cases
    lib = ctx._lib
    with open(os.path.join(_HERE, "golden", "key_blob", "k1_pk.bin"), "rb") as f:
        toy = g16.ProvingKey(ctx, f.read())
    out = {}

    def note(name, code):
        assert name not in out, name
        out[name] = [int(code), lib.og_last_error().decode("utf-8") if code else ""]

    def le(v):
        return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)

    rs, proofs = np.zeros((4, 64), dtype=np.uint8), np.zeros((4, 256), dtype=np.uint8)
    shp = (C.c_uint64 * 3)()

    # ---- withdraw -------------------------------------------------------------------------------------------------------------
    good = np.stack([circuit.pack_inputs(11 + k, 21 + k, 1000, 5, 31 + k, k % 4, [100 + 10 * k, 101 + 10 * k], token=7, chain_id=1)
                     for k in range(4)])
    assert lib.og_withdraw_shape(DEPTH, 0, 0, shp) == 0
    wit = np.zeros((4, int(shp[0]), 32), dtype=np.uint8)
    pk = withdraw_cases._key(ctx, DEPTH, 0, 0)[3]
    job = C.c_void_p()

    def w_witness(recs, depth=DEPTH, n=None):
        return lib.og_withdraw_witness_d(ctx._h, depth, 0, 0, ctx.ptr(recs), recs.shape[0] if n is None else n, ctx.ptr(wit))

    def w_prove(key, recs, depth=DEPTH, n=None):
        return lib.og_withdraw_prove_batch_d(ctx._h, key, depth, 0, 0, ctx.ptr(recs), recs.shape[0] if n is None else n, ctx.ptr(rs),
                                             ctx.ptr(proofs), None)

    def w_submit(key, recs, depth=DEPTH):
        """submit, and wait where a job came back: the refusal of a call that stays enqueued arrives at the wait"""
        rc = lib.og_withdraw_prove_batch_submit_d(ctx._h, key, depth, 0, 0, ctx.ptr(recs), recs.shape[0], ctx.ptr(rs), ctx.ptr(proofs), None,
                                                  C.byref(job))
        return lib.og_job_wait(ctx._h, job) if rc == 0 else rc

    def w_partials(key, recs, depth=DEPTH, n=None, rank=0, world=1):
        part = np.zeros((4, 768), dtype=np.uint8)
        return lib.og_withdraw_prove_partials_d(ctx._h, key, depth, 0, 0, ctx.ptr(recs), recs.shape[0] if n is None else n, rank, world,
                                                ctx.ptr(part), None)

    bad = [("field 0 of record 1 = r", 1, 0, R)]
    bad += [(f"sibling {lvl} = r", 2, W_REC + lvl, R) for lvl in range(DEPTH)]
    bad += [("index outside the tree", 2, 5, 1 << DEPTH)]
    for what, rec, field, value in bad:
        x = good.copy()
        x[rec, field] = le(value)
        note(f"withdraw: witness_d: {what}", w_witness(x))
        with _env(OG_GEN_ONE_SUB="0"):   # as a slab: refused before anything is proved
            note(f"withdraw: prove_batch_d, slab: {what}", w_prove(pk._h, x))
            note(f"withdraw: prove_batch_submit_d, slab: {what}", w_submit(pk._h, x))
            note(f"withdraw: prove_partials_d, slab: {what}", w_partials(pk._h, x))
    two = good[:2].copy()                # inside the pipeline (a proof costs seconds here: two records, one call per format)
    two[1, 0] = le(R)
    note("withdraw: prove_batch_d, in the pipeline: field 0 of record 1 = r", w_prove(pk._h, two))
    two = good[:2].copy()
    two[0, W_REC + 1] = le(R)
    note("withdraw: prove_batch_submit_d, in the pipeline: sibling 1 of record 0 = r", w_submit(pk._h, two))
    note("withdraw: witness_d n = 65536", w_witness(good, n=65536))
    for depth in (0, 65):
        note(f"withdraw: shape depth {depth}", lib.og_withdraw_shape(depth, 0, 0, shp))
        note(f"withdraw: witness_d depth {depth}", w_witness(good, depth=depth))
        note(f"withdraw: witness_d depth {depth}, n = 0", w_witness(good, depth=depth, n=0))
        note(f"withdraw: prove_batch_d depth {depth}", w_prove(toy._h, good, depth=depth))
        note(f"withdraw: prove_batch_d depth {depth}, n = 0", w_prove(toy._h, good, depth=depth, n=0))
        note(f"withdraw: prove_batch_submit_d depth {depth}", w_submit(toy._h, good, depth=depth))
        note(f"withdraw: prove_partials_d depth {depth}", w_partials(toy._h, good, depth=depth))
    note("withdraw: shape too many wires", lib.og_withdraw_shape(DEPTH, 1 << 30, 0, shp))
    note("withdraw: witness_d too many wires", lib.og_withdraw_witness_d(ctx._h, DEPTH, 1 << 30, 0, ctx.ptr(good), 4, ctx.ptr(wit)))
    note("withdraw: shape null", lib.og_withdraw_shape(DEPTH, 0, 0, None))
    note("withdraw: witness_d null ctx", lib.og_withdraw_witness_d(None, DEPTH, 0, 0, ctx.ptr(good), 4, ctx.ptr(wit)))
    if branch_only:
        note("withdraw: witness_d null inputs" + BRANCH_ONLY, lib.og_withdraw_witness_d(ctx._h, DEPTH, 0, 0, None, 4, ctx.ptr(wit)))
        note("withdraw: witness_d null output" + BRANCH_ONLY, lib.og_withdraw_witness_d(ctx._h, DEPTH, 0, 0, ctx.ptr(good), 4, None))
    note("withdraw: witness_d null pointers, n = 0", lib.og_withdraw_witness_d(ctx._h, DEPTH, 0, 0, None, 0, None))
    for name, entry in (("prove_batch_d", lib.og_withdraw_prove_batch_d), ("prove_batch_submit_d", lib.og_withdraw_prove_batch_submit_d)):
        tail = (C.byref(job),) if entry is lib.og_withdraw_prove_batch_submit_d else ()
        g, r, p = ctx.ptr(good), ctx.ptr(rs), ctx.ptr(proofs)
        note(f"withdraw: {name} null ctx", entry(None, pk._h, DEPTH, 0, 0, g, 4, r, p, None, *tail))
        note(f"withdraw: {name} null key", entry(ctx._h, None, DEPTH, 0, 0, g, 4, r, p, None, *tail))
        note(f"withdraw: {name} null inputs", entry(ctx._h, pk._h, DEPTH, 0, 0, None, 4, r, p, None, *tail))
        note(f"withdraw: {name} null rs", entry(ctx._h, pk._h, DEPTH, 0, 0, g, 4, None, p, None, *tail))
        note(f"withdraw: {name} null proofs", entry(ctx._h, pk._h, DEPTH, 0, 0, g, 4, r, None, None, *tail))
        note(f"withdraw: {name} null pointers, n = 0", entry(ctx._h, pk._h, DEPTH, 0, 0, None, 0, None, None, None, *tail))
    note("withdraw: prove_batch_submit_d null job_out",
         lib.og_withdraw_prove_batch_submit_d(ctx._h, pk._h, DEPTH, 0, 0, ctx.ptr(good), 4, ctx.ptr(rs), ctx.ptr(proofs), None, None))
    part = np.zeros((4, 768), dtype=np.uint8)
    note("withdraw: prove_partials_d null ctx", lib.og_withdraw_prove_partials_d(None, pk._h, DEPTH, 0, 0, ctx.ptr(good), 4, 0, 1, ctx.ptr(part), None))
    note("withdraw: prove_partials_d null key", w_partials(None, good))
    note("withdraw: prove_partials_d null inputs", lib.og_withdraw_prove_partials_d(ctx._h, pk._h, DEPTH, 0, 0, None, 4, 0, 1, ctx.ptr(part), None))
    note("withdraw: prove_partials_d null partials", lib.og_withdraw_prove_partials_d(ctx._h, pk._h, DEPTH, 0, 0, ctx.ptr(good), 4, 0, 1, None, None))
    note("withdraw: prove_partials_d n = 0", w_partials(pk._h, good, n=0))
    note("withdraw: prove_partials_d rank = world", w_partials(pk._h, good, rank=1, world=1))
    note("withdraw: prove_partials_d world = 0", w_partials(pk._h, good, rank=0, world=0))
    note("withdraw: prove_batch_d with a key of another statement", w_prove(toy._h, good))
    note("withdraw: prove_batch_submit_d with a key of another statement", w_submit(toy._h, good))
    note("withdraw: prove_partials_d with a key of another statement", w_partials(toy._h, good))
    with _env(OG_GEN_ONE_SUB="0"):
        note("withdraw: prove_batch_d, slab, with a key of another statement", w_prove(toy._h, good))
        note("withdraw: prove_batch_submit_d, slab, with a key of another statement", w_submit(toy._h, good))
    note("withdraw: well-formed records", w_witness(good))
    note("withdraw: prove_batch_d well-formed records", w_prove(pk._h, good[:2]))   # (two records: a proof costs seconds here)
    note("withdraw: prove_batch_submit_d well-formed records", w_submit(pk._h, good[:2]))
    with _env(OG_GEN_ONE_SUB="0"):
        note("withdraw: prove_batch_d, slab, well-formed records", w_prove(pk._h, good[:2]))

    # ---- deposit --------------------------------------------------------------------------------------------------------------
    dgood = np.stack([circuit.pack_deposit_inputs(11 + k, 21 + k, 31 + k) for k in range(4)])
    dblob, _vk = g16.setup(ctx, circuit.deposit_r1cs(ctx.mimc7_constants()), 41, 42, 43, 44, 45)
    dpk = g16.ProvingKey(ctx, dblob)
    assert lib.og_deposit_shape(shp) == 0
    dwit = np.zeros((4, int(shp[0]), 32), dtype=np.uint8)

    def d_witness(recs, n=None):
        return lib.og_deposit_witness_d(ctx._h, ctx.ptr(recs), recs.shape[0] if n is None else n, ctx.ptr(dwit))

    def d_prove(key, recs, n=None):
        return lib.og_deposit_prove_batch_d(ctx._h, key, ctx.ptr(recs), recs.shape[0] if n is None else n, ctx.ptr(rs), ctx.ptr(proofs), None)

    for field in range(3):
        x = dgood.copy()
        x[1 + field % 2, field] = le(R)
        note(f"deposit: witness_d: field {field} of record {1 + field % 2} = r", d_witness(x))
        note(f"deposit: prove_batch_d: field {field} of record {1 + field % 2} = r", d_prove(dpk._h, x))
    big = np.zeros((65536, 3, 32), dtype=np.uint8)   # (no refusal at the entry point: the records are checked, then the witness call refuses)
    note("deposit: witness_d n = 65536", lib.og_deposit_witness_d(ctx._h, ctx.ptr(big), 65536, ctx.ptr(dwit)))
    big[65535, 2] = le(R)
    note("deposit: witness_d n = 65536, field 2 of record 65535 = r", lib.og_deposit_witness_d(ctx._h, ctx.ptr(big), 65536, ctx.ptr(dwit)))
    note("deposit: shape null", lib.og_deposit_shape(None))
    note("deposit: witness_d null ctx", lib.og_deposit_witness_d(None, ctx.ptr(dgood), 4, ctx.ptr(dwit)))
    note("deposit: witness_d null inputs", lib.og_deposit_witness_d(ctx._h, None, 4, ctx.ptr(dwit)))
    note("deposit: witness_d null output", lib.og_deposit_witness_d(ctx._h, ctx.ptr(dgood), 4, None))
    note("deposit: witness_d null pointers, n = 0", lib.og_deposit_witness_d(ctx._h, None, 0, None))
    g, r, p = ctx.ptr(dgood), ctx.ptr(rs), ctx.ptr(proofs)
    note("deposit: prove_batch_d null ctx", lib.og_deposit_prove_batch_d(None, dpk._h, g, 4, r, p, None))
    note("deposit: prove_batch_d null key", lib.og_deposit_prove_batch_d(ctx._h, None, g, 4, r, p, None))
    note("deposit: prove_batch_d null inputs", lib.og_deposit_prove_batch_d(ctx._h, dpk._h, None, 4, r, p, None))
    note("deposit: prove_batch_d null rs", lib.og_deposit_prove_batch_d(ctx._h, dpk._h, g, 4, None, p, None))
    note("deposit: prove_batch_d null proofs", lib.og_deposit_prove_batch_d(ctx._h, dpk._h, g, 4, r, None, None))
    note("deposit: prove_batch_d with a key of another statement", d_prove(toy._h, dgood))
    note("deposit: prove_batch_d with a key of another statement, n = 0", d_prove(toy._h, dgood, n=0))
    note("deposit: well-formed records", d_witness(dgood))
    note("deposit: prove_batch_d well-formed records", d_prove(dpk._h, dgood[:2]))
    dpk.close()
    toy.close()
    return out


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_withdraw_deposit_errors(ectx):
    with open(_GOLDEN) as f:
        want = json.load(f)
    got = compute(ectx)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":
    from tests import emu
    res = compute(emu.Ctx(), branch_only="--before-the-table" not in sys.argv)
    with open(_GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
