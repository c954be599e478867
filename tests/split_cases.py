"""Split-statement cases shared by the CPU-interpreter run and the GPU run: the product's two R1CS builders and the HIP witness
kernel against the plain restatement in tests/split_spec.py, then proofs -- byte-identical to the C restatement's, accepted by
og_verify for the seven public inputs and refused for anything else --, the overdraw that must stay unprovable, and the boundary
check of the records."""
import random

import numpy as np
import pytest

from oracle.py import fields, mimc7
from oracle.py.withdraw import _CS, _hash2
from tests import split_spec as spec
from tests.withdraw_cases import _rows, _oracle_rows

R = fields.R
TOP = (1 << 128) - 1
_TOXIC = (15, 16, 17, 18, 19)
FIELDS = ("nullifier", "secret", "amount", "recipient", "amount_out", "index", "token", "chain_id", "change_commitment")


def _inputs(rnd, depth):
    amount = rnd.randrange(1, 1 << 64)
    return dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=amount, recipient=rnd.randrange(1 << 160),
                amount_out=rnd.randrange(amount + 1), index=rnd.randrange(1 << depth), siblings=[rnd.randrange(R) for _ in range(depth)],
                token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32), change_commitment=rnd.randrange(R))


def edge_inputs(rnd, depth, n):
    """n >= 3 requests; the first three carry, by construction: index 0 with amount_out = 0 (a transfer inside the pool); the last
    leaf with amount_out = amount = 2^128 - 1 (a zero-value change note, the largest note); amount = 2^128 - 1 with amount_out = 1
    and nullifier = secret = change_commitment = r - 1"""
    assert n >= 3
    ins = [_inputs(rnd, depth) for _ in range(n)]
    ins[0].update(index=0, amount_out=0)
    ins[1].update(index=(1 << depth) - 1, amount=TOP, amount_out=TOP)
    ins[2].update(amount=TOP, amount_out=1, nullifier=R - 1, secret=R - 1, change_commitment=R - 1)
    return ins


def _pack(circuit, i):
    return circuit.pack_split_inputs(**i)


def _spec(i, depth):
    return spec.build(depth, **i)


def _key(ctx, depth, statement="split"):
    """(key blob, vk, loaded key, close) of the split statement (or the natural withdraw statement) at `depth`.  On the CPU
    interpreter set-up and the key upload take tens of seconds, so there the cases of a session share one key per shape and
    `close` does nothing (as tests/withdraw_cases._key); on the GPU every case loads and frees its own."""
    from owshen_amd import circuit, groth16 as g16
    shared = type(ctx).__module__ == "tests.emu"
    cache = ctx.__dict__.setdefault("_split_keys", {}) if shared else {}
    k = (statement, depth)
    if k not in cache:
        r1 = circuit.split_r1cs(ctx.mimc7_constants(), depth) if statement == "split" else circuit.withdraw_r1cs(ctx.mimc7_constants(), depth)
        blob, vk = g16.setup(ctx, r1, *_TOXIC)
        cache[k] = (blob, vk, g16.ProvingKey(ctx, blob))
    blob, vk, pk = cache[k]
    return blob, vk, pk, (lambda: None) if shared else pk.close


def case_r1cs_and_witness_match_spec(ctx, depth, n, seed=1):
    """both builders give the spec's rows, og_split_shape is the spec's shape, and the kernel's witness is the spec's z integer for
    integer -- over the edge requests of `edge_inputs`"""
    import ctypes as C
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    ins = edge_inputs(rnd, depth, n)
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_split_shape(depth, shp))
    assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.split_shape(depth) and int(shp[2]) == spec.N_PUB == 7
    r1 = circuit.split_r1cs(ctx.mimc7_constants(), depth)
    nat = circuit.split_r1cs_native(ctx, depth)
    assert (nat.n_wires, nat.n_pub, nat.n_constraints, nat.log_d) == (r1.n_wires, r1.n_pub, r1.n_constraints, r1.log_d)
    assert (r1.n_wires, r1.n_constraints) == spec.shape(depth) and r1.n_pub == 7
    wit = ctx.to_host(circuit.split_witness(ctx, depth, ctx.to_device(np.stack([_pack(circuit, i) for i in ins]))))
    for k, i in enumerate(ins):
        m, l, cons, z = _spec(i, depth)
        assert (m, l) == (r1.n_wires, r1.n_pub) and len(cons) == r1.n_constraints
        assert api.bytes_to_ints(wit[k]) == z, f"split witness {k}"
        change = i["amount"] - i["amount_out"]
        leaf = mimc7.hash2(mimc7.hash2(i["nullifier"], i["secret"]), mimc7.hash2(i["amount"], i["token"]))
        assert z[1] == mimc7.merkle_root_from_path(leaf, i["index"], i["siblings"])[-1] and z[2] == mimc7.hash2(i["nullifier"], 0)
        assert z[3:7] == [i["recipient"], i["amount_out"], i["token"], i["chain_id"]] and z[12] == change
        assert z[7] == mimc7.hash2(i["change_commitment"], mimc7.hash2(change, i["token"])), "change_leaf"
        if k == 0:
            ident, empty = [[(w, 1)] for w in range(l + 1)], [[] for _ in range(l + 1)]
            for name, which, extra in (("a", 0, ident), ("b", 1, empty), ("c", 2, empty)):
                assert _rows(getattr(r1, name)) == _oracle_rows(cons, which, extra), name
                assert _rows(getattr(nat, name)) == _rows(getattr(r1, name)), name
    # the ledger's side: the change leaf through og_mimc7_hash2_d
    i = ins[2]
    assert circuit.split_change_leaf(i["change_commitment"], i["amount"] - i["amount_out"], i["token"], ctx) == _spec(i, depth)[3][7]


def case_split_end_to_end(ctx, depth, n=4, seed=2, key=None):
    """records -> proofs: the C restatement's bytes, the generic prover's bytes from the generated witnesses, og_verify accepts the
    seven returned inputs and refuses amount_out + 1, another change_leaf, another recipient, another root"""
    from oracle.c import binding as oc
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    ins = edge_inputs(rnd, depth, max(n, 3))[:n]
    recs = np.stack([_pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    proofs, pub = circuit.split_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True)
    wit_d = circuit.split_witness(ctx, depth, ctx.to_device(recs))
    wit = ctx.to_host(wit_d)
    assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:8]).tobytes()
    assert circuit.split_prove(ctx, pk, depth, ctx.to_device(recs), rs).tobytes() == proofs.tobytes()       # public_out = NULL
    assert pk.prove_batch_device(wit_d, rs).tobytes() == proofs.tobytes()                                  # the generic entry point
    ck = oc.prepared_key_from_blob(blob)
    vkb = g16.vk_to_bytes(vk)
    lib = ctx._lib
    for t, i in enumerate(ins):
        assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"split proof {t} differs from the C restatement"
        z = _spec(i, depth)[3]
        good = api.bytes_to_ints(pub[t])
        assert good == z[1:8] and good[3] == i["amount_out"]
        p = proofs[t].tobytes()
        assert g16.verify(vkb, good, p, lib=lib) is True
        for slot in (3, 6, 2, 0):          # amount_out + 1, another change_leaf, another recipient, another root
            forged = list(good)
            forged[slot] = (forged[slot] + 1) % R
            assert g16.verify(vkb, forged, p, lib=lib) is False, slot
    assert g16.verify(vkb, pub[1], proofs[0].tobytes(), lib=lib) is False
    close()


def _gadget_wires(l, r, with_out):
    """the wires one MultiMiMC7 gadget allocates for inputs (l, r), and its output (the spec's own gadget)"""
    cs = _CS()
    wl, wr = cs.alloc(l), cs.alloc(r)
    out = mimc7.hash2(l, r)
    if with_out:
        _hash2(cs, {wl: 1}, {wr: 1})
        return cs.z[3:], out
    wo = cs.alloc(out)
    _hash2(cs, {wl: 1}, {wr: 1}, out_wire=wo)
    return cs.z[4:], out


def forge_overdraw(depth, i):
    """(z, rows that fail): a valid witness of request i turned into an overdraw -- amount_out = amount + 1 and change = r - 1 =
    -1, so that amount_out + change = amount still holds in the field; the bit wires are those of the low 128 bits of both values
    and the two change hashes are recomputed, so every row holds except the recomposition of `change`"""
    m, _l, cons, z = _spec(i, depth)
    z = list(z)
    out, change = i["amount"] + 1, R - 1
    assert out < (1 << 128)
    z[4], z[12] = out, change
    b0 = 13 + 2 * depth + 2
    for k in range(128):
        z[b0 + k] = (out >> k) & 1
        z[b0 + 128 + k] = (change >> k) & 1
    asset_wires, asset = _gadget_wires(change, i["token"], True)
    leaf_wires, leaf = _gadget_wires(i["change_commitment"], asset, False)
    assert len(asset_wires) == 730 and len(leaf_wires) == 729
    z[m - 1459:m - 729] = asset_wires
    z[m - 729:] = leaf_wires
    z[7] = leaf
    assert len(z) == m

    def val(lc):
        return sum(c * z[w] for w, c in lc.items()) % R

    failing = [k for k, (a, b, c) in enumerate(cons) if val(a) * val(b) % R != val(c)]
    return z, failing


def case_overdraw_is_unprovable(ctx, depth, seed=3, key=None):
    """a forged overdraw fails the range rows alone: og_prove_batch_d answers OG_ERR_UNSATISFIED; the same request as a record is
    OG_ERR_INVALID naming field 4"""
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    i = _inputs(rnd, depth)
    z, failing = forge_overdraw(depth, i)
    assert failing == [3 + 129 + 128], failing      # the recomposition row of `change` and nothing else
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    wit = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(1, -1, 32).copy()
    with pytest.raises(api.OwshenGpuError) as e:
        pk.prove_batch_device(ctx.to_device(wit), rs)
    assert e.value.code == -4, str(e.value)
    # (the witness it was forged from proves)
    good = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in _spec(i, depth)[3]), dtype=np.uint8).reshape(1, -1, 32).copy()
    assert pk.prove_batch_device(ctx.to_device(good), rs).shape == (1, 256)
    over = dict(i, amount_out=i["amount"] + 1)
    for call in (lambda d: circuit.split_prove(ctx, pk, depth, d, rs), lambda d: circuit.split_witness(ctx, depth, d)):
        with pytest.raises(api.OwshenGpuError) as e:
            call(ctx.to_device(_pack(circuit, over)[None]))
        assert e.value.code == -1 and "input record 0: field 4 (amount_out)" in str(e.value), str(e.value)
    close()


def case_record_boundary(ctx, depth, seed=4, key=None, other_keys=True):
    """one bad field per case: OG_ERR_INVALID names the record and its lowest offending field, from og_split_witness_d and from
    og_split_prove_batch_d; the largest well-formed values pass; keys of another shape are refused"""
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    nrec = 4
    ins = [_inputs(rnd, depth) for _ in range(nrec)]
    good = np.stack([_pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]

    def le(v):
        return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)

    def with_fields(rec, **fv):
        x = good.copy()
        for name, value in fv.items():
            x[rec, FIELDS.index(name) if name in FIELDS else 9 + int(name[1:])] = le(value)
        return x

    bad_cases = [
        (with_fields(3, secret=R), 3, 1, "secret"),
        (with_fields(1, amount=1 << 128), 1, 2, "amount"),
        (with_fields(2, amount=(1 << 128) + 5, amount_out=1 << 128), 2, 2, "amount"),       # two fields offend: the lowest is named
        (with_fields(0, amount_out=ins[0]["amount"] + 1), 0, 4, "amount_out"),
        (with_fields(3, index=1 << depth), 3, 5, "index"),
        (with_fields(2, **{f"s{depth - 1}": R}), 2, 9 + depth - 1, f"sibling {depth - 1}"),
    ]
    for k, (packed, rec, field, name) in enumerate(bad_cases):
        for call in (lambda d: circuit.split_witness(ctx, depth, d), lambda d: circuit.split_prove(ctx, pk, depth, d, rs)):
            with pytest.raises(api.OwshenGpuError) as e:
                call(ctx.to_device(packed))
            assert e.value.code == -1 and f"input record {rec}: field {field} ({name})" in str(e.value), str(e.value)
    # the largest well-formed values pass the boundary
    edge = with_fields(0, nullifier=R - 1, amount=TOP, amount_out=TOP, index=(1 << depth) - 1, change_commitment=R - 1)
    circuit.split_witness(ctx, depth, ctx.to_device(edge))
    if other_keys:
        for statement, d in (("withdraw", depth), ("split", depth + 1 if depth == 1 else depth - 1)):
            _b, _v, other, close_other = _key(ctx, d, statement)
            with pytest.raises(api.OwshenGpuError) as e:
                circuit.split_prove(ctx, other, depth, ctx.to_device(good), rs)
            assert e.value.code == -1 and "not for this split-statement shape" in str(e.value), str(e.value)
            close_other()
    close()
