"""Every refusal of the split, join and transfer entry points, byte for byte: return code and the full og_last_error() text, on the
CPU interpreter at depth 2, against tests/golden/record_statement_errors.json.

The texts are a recording (`python -m tests.test_record_statement_errors` writes them), made while each statement still formatted
its own messages; the boundary cases of tests/*_cases.py pin substrings only.  Per statement: field 0 of record 1 set to r, a
sibling set to r (on either path of join), an index of 1 << depth, the failures of the amount relation, 65536 records, depth 0 and
65 and a null argument at each of og_<st>_shape / _witness_d / _prove_batch_d / _r1cs, and a key of another statement (the toy key
of tests/golden/key_blob)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_GOLDEN = os.path.join(_HERE, "golden", "record_statement_errors.json")
DEPTH = 2
N_REC = {"split": 9, "join": 11, "transfer": 9}   # fields before the siblings
PATHS = {"split": 1, "join": 2, "transfer": 1}


def _good(circuit, st, k):
    """record k of a well-formed batch (small distinct values: nothing here depends on them)"""
    sib = [100 + 10 * k, 101 + 10 * k]
    if st == "split":
        return circuit.pack_split_inputs(11 + k, 21 + k, 1000, 5, 400, k % 4, sib, token=7, chain_id=1, change_commitment=31 + k)
    if st == "join":
        return circuit.pack_join_inputs(11 + k, 21 + k, 1000, k % 4, sib, 41 + k, 51 + k, 2000, (k + 1) % 4, [s + 50 for s in sib], token=7,
                                        chain_id=1, out_commitment=31 + k)
    return circuit.pack_transfer_inputs(11 + k, 21 + k, 1000, k % 4, sib, token=7, chain_id=1, pay_commitment=61 + k, pay_amount=400,
                                        change_commitment=31 + k)


# field numbers of the records (include/owshen_gpu.h)
_BAD_RECORDS = {
    "split": [("index outside the tree", 2, 5, 1 << DEPTH), ("amount_out > amount", 0, 4, 1001), ("amount >= 2^128", 3, 2, 1 << 128)],
    "join": [("index_a outside the tree", 2, 3, 1 << DEPTH), ("index_b outside the tree", 2, 7, 1 << DEPTH),
             ("amount_a + amount_b >= 2^128", 0, 6, (1 << 128) - 1000), ("amount_a >= 2^128", 3, 2, 1 << 128),
             ("nullifier_b = nullifier_a", 1, 4, 12)],
    "transfer": [("index outside the tree", 2, 3, 1 << DEPTH), ("pay_amount > amount", 0, 7, 1001), ("amount >= 2^128", 3, 2, 1 << 128)],
}


def compute(ctx):
    from owshen_amd import circuit, groth16 as g16
    from owshen_amd.api import FR_MODULUS as R
    lib = ctx._lib
    with open(os.path.join(_HERE, "golden", "key_blob", "k1_pk.bin"), "rb") as f:
        toy = g16.ProvingKey(ctx, f.read())
    out = {}

    def note(name, code):
        out[name] = [int(code), lib.og_last_error().decode("utf-8") if code else ""]

    def le(v):
        return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)

    for st in ("split", "join", "transfer"):
        shape, witness, prove, r1cs = (getattr(lib, f"og_{st}_{f}") for f in ("shape", "witness_d", "prove_batch_d", "r1cs"))
        good = np.stack([_good(circuit, st, k) for k in range(4)])
        shp = (C.c_uint64 * 3)()
        assert shape(DEPTH, shp) == 0
        wit = np.zeros((4, int(shp[0]), 32), dtype=np.uint8)
        rs, proofs = np.zeros((4, 64), dtype=np.uint8), np.zeros((4, 256), dtype=np.uint8)
        h = C.c_void_p()

        def run_witness(recs, depth=DEPTH, n=None):
            return witness(ctx._h, depth, ctx.ptr(recs), recs.shape[0] if n is None else n, ctx.ptr(wit))

        def run_prove(pk, recs, depth=DEPTH):
            return prove(ctx._h, pk, depth, ctx.ptr(recs), recs.shape[0], ctx.ptr(rs), ctx.ptr(proofs), None)

        bad = [("field 0 of record 1 = r", 1, 0, R)]
        bad += [(f"sibling {lvl} of path {p} = r", 2, N_REC[st] + p * DEPTH + lvl, R) for p in range(PATHS[st]) for lvl in range(DEPTH)]
        for what, rec, field, value in bad + _BAD_RECORDS[st]:
            x = good.copy()
            x[rec, field] = le(value)
            note(f"{st}: {what}", run_witness(x))
        note(f"{st}: witness_d n = 65536", run_witness(good, n=65536))
        for depth in (0, 65):
            note(f"{st}: shape depth {depth}", shape(depth, shp))
            note(f"{st}: witness_d depth {depth}", run_witness(good, depth=depth))
            note(f"{st}: prove_batch_d depth {depth}", run_prove(toy._h, good, depth=depth))
            note(f"{st}: r1cs depth {depth}", r1cs(ctx._h, depth, C.byref(h)))
        note(f"{st}: shape null", shape(DEPTH, None))
        note(f"{st}: witness_d null ctx", witness(None, DEPTH, ctx.ptr(good), 4, ctx.ptr(wit)))
        note(f"{st}: witness_d null inputs", witness(ctx._h, DEPTH, None, 4, ctx.ptr(wit)))
        note(f"{st}: witness_d null output", witness(ctx._h, DEPTH, ctx.ptr(good), 4, None))
        note(f"{st}: prove_batch_d null ctx", prove(None, toy._h, DEPTH, ctx.ptr(good), 4, ctx.ptr(rs), ctx.ptr(proofs), None))
        note(f"{st}: prove_batch_d null key", run_prove(None, good))
        note(f"{st}: prove_batch_d null inputs", prove(ctx._h, toy._h, DEPTH, None, 4, ctx.ptr(rs), ctx.ptr(proofs), None))
        note(f"{st}: prove_batch_d null rs", prove(ctx._h, toy._h, DEPTH, ctx.ptr(good), 4, None, ctx.ptr(proofs), None))
        note(f"{st}: prove_batch_d null proofs", prove(ctx._h, toy._h, DEPTH, ctx.ptr(good), 4, ctx.ptr(rs), None, None))
        note(f"{st}: r1cs null ctx", r1cs(None, DEPTH, C.byref(h)))
        note(f"{st}: r1cs null out", r1cs(ctx._h, DEPTH, None))
        note(f"{st}: prove_batch_d with a key of another statement", run_prove(toy._h, good))
        note(f"{st}: well-formed records", run_witness(good))
    toy.close()
    return out


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_record_statement_errors(ectx):
    from tests import transfer_cases
    with open(_GOLDEN) as f:
        want = json.load(f)
    with transfer_cases.walk(**transfer_cases.LANE_LOCAL):   # (the one call that reaches a walk: the well-formed records)
        got = compute(ectx)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":
    from tests import emu, transfer_cases
    with transfer_cases.walk(**transfer_cases.LANE_LOCAL):
        res = compute(emu.Ctx())
    with open(_GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
