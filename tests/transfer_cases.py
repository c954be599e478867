"""Transfer-statement cases shared by the CPU-interpreter run and the GPU run: the product's two R1CS builders and the HIP witness
kernels -- the lane-local walk and the wave-wide one -- against the plain restatement in tests/transfer_spec.py, then proofs --
byte-identical to the C restatement's, accepted for the five public inputs and refused for anything else --, four forged witnesses
that must stay unprovable, the boundary check of the records, and the two new notes spent again by `withdraw` and `split`."""
import contextlib
import os
import random

import numpy as np
import pytest

from oracle.py import fields, mimc7, withdraw as withdraw_spec
from tests import split_spec, transfer_spec as spec
from tests.withdraw_cases import _rows, _oracle_rows

R = fields.R
TOP = (1 << 128) - 1
_TOXIC = (25, 26, 27, 28, 29)
FIELDS = ("nullifier", "secret", "amount", "index", "token", "chain_id", "pay_commitment", "pay_amount", "change_commitment")
_WALK_ENV = ("OG_WITNESS_W9", "OG_WITNESS_W9_MAX", "OG_W9_ROWS")
LANE_LOCAL = {"OG_WITNESS_W9": "0"}


@contextlib.contextmanager
def walk(**env):
    """the hooks that choose the witness walk (read per call by the hooks build and the interpreter build, never by the shipped
    library), set for the block and put back after it"""
    saved = {k: os.environ.get(k) for k in _WALK_ENV}
    for k in _WALK_ENV:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _inputs(rnd, depth, **values):
    amount = rnd.randrange(1, 1 << 64)
    i = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=amount, index=rnd.randrange(1 << depth),
             siblings=[rnd.randrange(R) for _ in range(depth)], token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32),
             pay_commitment=rnd.randrange(R), pay_amount=rnd.randrange(amount + 1), change_commitment=rnd.randrange(R))
    i.update(values)
    return i


def edge_inputs(rnd, depth, n):
    """n >= 5 requests; the first five carry, by construction: index 0 (the all-left walk: every permutation of the levels is on the
    chain) with pay_amount = 0; the last leaf (the all-right walk: every level's first permutation comes from the first launch) with
    pay_amount = amount = 2^128 - 1; amount = 2^128 - 1 with pay_amount = 1 and nullifier = secret = pay_commitment = r - 1;
    pay_commitment = change_commitment; pay_amount = amount (a zero-value change note)"""
    assert n >= 5
    ins = [_inputs(rnd, depth) for _ in range(n)]
    ins[0].update(index=0, pay_amount=0)
    ins[1].update(index=(1 << depth) - 1, amount=TOP, pay_amount=TOP)
    ins[2].update(amount=TOP, pay_amount=1, nullifier=R - 1, secret=R - 1, pay_commitment=R - 1)
    ins[3].update(change_commitment=ins[3]["pay_commitment"])
    ins[4].update(pay_amount=ins[4]["amount"])
    return ins


def _pack(circuit, i):
    return circuit.pack_transfer_inputs(**i)


def _spec(i, depth, forge=None):
    return spec.build(depth, forge=forge, **i)


def _wit_bytes(z):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(1, -1, 32).copy()


def _key(ctx, depth, statement="transfer"):
    """(key blob, vk, loaded key, close) of the transfer statement (or of split / join / the natural withdraw statement) at `depth`.
    On the CPU interpreter set-up and the key upload take tens of seconds, so there the cases of a session share one key per shape
    and `close` does nothing (as tests/split_cases._key); on the GPU every case loads and frees its own."""
    from owshen_amd import circuit, groth16 as g16
    shared = type(ctx).__module__ == "tests.emu"
    cache = ctx.__dict__.setdefault("_transfer_keys", {}) if shared else {}
    k = (statement, depth)
    if k not in cache:
        r1 = getattr(circuit, statement + "_r1cs")(ctx.mimc7_constants(), depth)
        blob, vk = g16.setup(ctx, r1, *_TOXIC)
        cache[k] = (blob, vk, g16.ProvingKey(ctx, blob))
    blob, vk, pk = cache[k]
    return blob, vk, pk, (lambda: None) if shared else pk.close


def _check_witness(api, got_bytes, z, what):
    got = api.bytes_to_ints(got_bytes)
    assert got == z, f"{what}: first differing wire {next(w for w in range(len(z)) if got[w] != z[w])}"


def case_r1cs_and_witness_match_spec(ctx, depth, n, seed=1):
    """both builders give the spec's rows, og_transfer_shape is the spec's shape, and the witness of the call's default walk is the
    spec's z integer for integer -- over the edge requests of `edge_inputs`"""
    import ctypes as C
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    ins = edge_inputs(rnd, depth, n)
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_transfer_shape(depth, shp))
    assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.transfer_shape(depth) and int(shp[2]) == spec.N_PUB == 5
    r1 = circuit.transfer_r1cs(ctx.mimc7_constants(), depth)
    nat = circuit.transfer_r1cs_native(ctx, depth)
    assert (nat.n_wires, nat.n_pub, nat.n_constraints, nat.log_d) == (r1.n_wires, r1.n_pub, r1.n_constraints, r1.log_d)
    assert (r1.n_wires, r1.n_constraints) == spec.shape(depth) and r1.n_pub == 5
    wit = ctx.to_host(circuit.transfer_witness(ctx, depth, ctx.to_device(np.stack([_pack(circuit, i) for i in ins]))))
    for k, i in enumerate(ins):
        m, l, cons, z = _spec(i, depth)
        assert (m, l) == (r1.n_wires, r1.n_pub) and len(cons) == r1.n_constraints
        _check_witness(api, wit[k], z, f"transfer witness {k}")
        change = i["amount"] - i["pay_amount"]
        leaf = mimc7.hash2(mimc7.hash2(i["nullifier"], i["secret"]), mimc7.hash2(i["amount"], i["token"]))
        assert z[1] == mimc7.merkle_root_from_path(leaf, i["index"], i["siblings"])[-1] and z[2] == mimc7.hash2(i["nullifier"], 0)
        assert z[3] == i["chain_id"] and z[9] == i["token"] and z[11] + z[13] == i["amount"] and z[13] == change
        assert z[4] == mimc7.hash2(i["pay_commitment"], mimc7.hash2(i["pay_amount"], i["token"])), "pay_leaf"
        assert z[5] == mimc7.hash2(i["change_commitment"], mimc7.hash2(change, i["token"])), "change_leaf"
        if k == 0:
            ident, empty = [[(w, 1)] for w in range(l + 1)], [[] for _ in range(l + 1)]
            for name, which, extra in (("a", 0, ident), ("b", 1, empty), ("c", 2, empty)):
                assert _rows(getattr(r1, name)) == _oracle_rows(cons, which, extra), name
                assert _rows(getattr(nat, name)) == _rows(getattr(r1, name)), name
    # the ledger's and the payee's side: both leaves through og_mimc7_hash2_d
    i = ins[2]
    z = _spec(i, depth)[3]
    assert circuit.transfer_leaves(i["pay_commitment"], i["pay_amount"], i["change_commitment"], i["amount"] - i["pay_amount"], i["token"],
                                   ctx) == (z[4], z[5])


def case_walks_agree(ctx, depth, ins):
    """the lane-local walk and the wave-wide walk in each of its three round forms, forced through OG_WITNESS_W9 / OG_W9_ROWS and
    chosen through OG_WITNESS_W9_MAX at n - 1 (lane-local) and at n (wave-wide): the spec's bytes every time.  `ctx` reads the hooks."""
    from owshen_amd import circuit
    n = len(ins)
    recs = np.stack([_pack(circuit, i) for i in ins])
    want = np.concatenate([_wit_bytes(_spec(i, depth)[3]) for i in ins]).tobytes()
    settings = [dict(OG_WITNESS_W9=0)] + [dict(OG_WITNESS_W9=1, OG_W9_ROWS=rows) for rows in (0, 1, 2)]
    settings += [dict(OG_WITNESS_W9_MAX=n - 1), dict(OG_WITNESS_W9_MAX=n)]
    for env in settings:
        with walk(**env):
            got = ctx.to_host(circuit.transfer_witness(ctx, depth, ctx.to_device(recs)))
        assert got.tobytes() == want, env


def case_transfer_end_to_end(ctx, depth, n=4, seed=2, key=None):
    """records -> proofs: the C restatement's bytes, the generic prover's bytes from the generated witnesses; og_verify and
    og_verify_batch_d (under og_vk_load, n_pub = 5) accept the five returned inputs; refused with pay_leaf and change_leaf exchanged,
    with any one input changed, and with a neighbour's inputs"""
    from oracle.c import binding as oc
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    ins = edge_inputs(rnd, depth, 5)[:n]
    recs = np.stack([_pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    proofs, pub = circuit.transfer_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True)
    wit_d = circuit.transfer_witness(ctx, depth, ctx.to_device(recs))
    wit = ctx.to_host(wit_d)
    assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:6]).tobytes()
    assert circuit.transfer_prove(ctx, pk, depth, ctx.to_device(recs), rs).tobytes() == proofs.tobytes()    # public_out = NULL
    assert pk.prove_batch_device(wit_d, rs).tobytes() == proofs.tobytes()                                  # the generic entry point
    ck = oc.prepared_key_from_blob(blob)
    vkb = g16.vk_to_bytes(vk)
    lib = ctx._lib
    for t, i in enumerate(ins):
        assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"transfer proof {t} differs from the C restatement"
        z = _spec(i, depth)[3]
        good = api.bytes_to_ints(pub[t])
        assert good == z[1:6]
        p = proofs[t].tobytes()
        assert g16.verify(vkb, good, p, lib=lib) is True
        assert good[3] != good[4]
        assert g16.verify(vkb, good[:3] + [good[4], good[3]], p, lib=lib) is False, "pay_leaf and change_leaf exchanged"
        for slot in range(5):          # root, nullifier_hash, chain_id, pay_leaf, change_leaf: each + 1
            forged = list(good)
            forged[slot] = (forged[slot] + 1) % R
            assert g16.verify(vkb, forged, p, lib=lib) is False, slot
    assert g16.verify(vkb, pub[1], proofs[0].tobytes(), lib=lib) is False
    with g16.VerifyingKey(ctx, vkb) as dvk:
        assert dvk.n_pub == 5
        assert dvk.verify_batch(pub, proofs).all()
        swapped = np.ascontiguousarray(pub[:, (0, 1, 2, 4, 3)])
        assert not dvk.verify_batch(swapped, proofs).any()
        assert not dvk.verify_batch(np.roll(pub, 1, axis=0), proofs).any()       # every proof against a neighbour's inputs
    close()


def _failing(cons, z):
    def val(lc):
        return sum(c * z[w] for w, c in lc.items()) % R

    return [k for k, (a, b, c) in enumerate(cons) if val(a) * val(b) % R != val(c)]


def forgeries(rnd, depth):
    """(honest request, [(name, z, the rows that must fail)]): four witnesses that are wrong in one place each, every other wire
    what an honest prover's would be (tests/transfer_spec.py build(forge=...)).
    created value: change = amount - pay_amount + 1 with its bits and the change gadgets following -- only the sum row fails;
    the wrap: pay_amount = amount + 1 and change = r - 1 = -1, so the sum holds in the field; the bit wires are the low 128 bits and
      all four output gadgets follow -- only the recomposition of `change`, the last of its range rows, fails;
    a pay_leaf for a larger amount: wire 4 = H(pay_commitment, H(pay_amount + 1, token)) over honest gadgets -- only the output
      row of the pay_leaf gadget fails;
    pay_asset formed with another token: the gadget's values are H(pay_amount, token')'s and pay_leaf follows, but its rows name
      the ONE token wire -- the two rows of the second permutation's first round that read the right input (t^2 and t^7; its t^4
      and t^6 rows hold between the forged wires) and the gadget's output row fail"""
    honest = _inputs(rnd, depth)
    change = honest["amount"] - honest["pay_amount"]
    m, _l, cons, _z = _spec(honest, depth)
    out = [("created value", _spec(honest, depth, forge={"change": change + 1})[3], [spec.ROW_SUM])]
    wrapped = dict(honest, pay_amount=honest["amount"] + 1)
    z = _spec(wrapped, depth, forge={})[3]
    assert z[11] == honest["amount"] + 1 and z[13] == R - 1
    out.append(("the wrap", z, [spec.ROW_CHANGE_RANGE]))
    larger = mimc7.hash2(honest["pay_commitment"], mimc7.hash2(honest["pay_amount"] + 1, honest["token"]))
    out.append(("a pay_leaf for a larger amount", _spec(honest, depth, forge={"pay_leaf": larger})[3],
                [spec.gadget_row(depth, 5 + depth) + 729]))
    g = spec.gadget_row(depth, 4 + depth)
    out.append(("pay_asset formed with another token", _spec(honest, depth, forge={"pay_asset_token": honest["token"] + 1})[3],
                [g + 365, g + 368, g + 729]))
    for name, z, rows in out:
        assert len(z) == m and _failing(cons, z) == rows, (name, _failing(cons, z), rows)
    return honest, out


def case_forgeries_are_unprovable(ctx, depth, seed=3, key=None):
    """each forged witness fails exactly its rows on the CPU, and og_prove_batch_d answers OG_ERR_UNSATISFIED for it; the honest
    witness proves"""
    from owshen_amd import api
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    honest, forged = forgeries(rnd, depth)
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    for name, z, _rows_failing in forged:
        with pytest.raises(api.OwshenGpuError) as e:
            pk.prove_batch_device(ctx.to_device(_wit_bytes(z)), rs)
        assert e.value.code == -4, (name, str(e.value))
    assert pk.prove_batch_device(ctx.to_device(_wit_bytes(_spec(honest, depth)[3])), rs).shape == (1, 256)
    close()


def case_record_boundary(ctx, depth, seed=4, key=None, other_keys=True):
    """one bad record per case: OG_ERR_INVALID names the record and its lowest offending field, from og_transfer_witness_d and from
    og_transfer_prove_batch_d; the largest well-formed record passes; a split key (another n_pub) and a join key (n_pub = 5, another
    wire count) are refused"""
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
        """s<l>: sibling l"""
        x = good.copy()
        for name, value in fv.items():
            x[rec, FIELDS.index(name) if name in FIELDS else 9 + int(name[1:])] = le(value)
        return x

    # every field >= r, each in another record (an `amount` or a `pay_amount` of r is also >= 2^128: the same field is named)
    bad_cases = [(with_fields(f % nrec, **{name: R}), f % nrec, f, name) for f, name in enumerate(FIELDS)]
    bad_cases += [(with_fields(1, **{f"s{l}": R}), 1, 9 + l, f"sibling {l}") for l in range(depth)]
    bad_cases += [
        (with_fields(3, index=1 << depth), 3, 3, "index"),
        (with_fields(1, amount=1 << 128, pay_amount=0), 1, 2, "amount"),
        (with_fields(2, amount=TOP, pay_amount=1 << 128), 2, 7, "pay_amount"),
        (with_fields(0, pay_amount=ins[0]["amount"] + 1), 0, 7, "pay_amount"),
        (with_fields(2, amount=(1 << 128) + 5, pay_amount=1 << 128, change_commitment=R), 2, 2, "amount"),   # three fields offend: the lowest is named
        (with_fields(3, pay_amount=ins[3]["amount"] + 1, **{f"s{depth - 1}": R}), 3, 7, "pay_amount"),
    ]
    for k, (packed, rec, field, name) in enumerate(bad_cases):
        for call in (lambda d: circuit.transfer_witness(ctx, depth, d), lambda d: circuit.transfer_prove(ctx, pk, depth, d, rs)):
            with pytest.raises(api.OwshenGpuError) as e:
                call(ctx.to_device(packed))
            assert e.value.code == -1 and f"input record {rec}: field {field} ({name})" in str(e.value), (k, str(e.value))
    # the largest well-formed record passes the boundary
    edge = with_fields(0, nullifier=R - 1, secret=R - 1, amount=TOP, index=(1 << depth) - 1, token=R - 1, chain_id=R - 1,
                       pay_commitment=R - 1, pay_amount=TOP, change_commitment=R - 1, **{f"s{depth - 1}": R - 1})
    circuit.transfer_witness(ctx, depth, ctx.to_device(edge))
    if other_keys:
        for statement in ("split", "join"):
            _b, _v, other, close_other = _key(ctx, depth, statement)
            assert other.n_pub == (7 if statement == "split" else 5)
            with pytest.raises(api.OwshenGpuError) as e:
                circuit.transfer_prove(ctx, other, depth, ctx.to_device(good), rs)
            assert e.value.code == -1 and "not for this transfer-statement shape" in str(e.value), str(e.value)
            close_other()
    close()


def case_notes_are_spendable(ctx, depth=4, seed=6):
    """a ledger in small: a note is deposited into a tree kept with og_mimc7_append_d, spent by `transfer`, both new leaves are
    appended, then the pay note is spent by `withdraw` and the change note by `split`, each under the new root -- all three proofs
    verify, and the nullifier hash the transfer publishes is the one `withdraw` would publish for the same note"""
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    lib = ctx._lib

    def tob(vals):
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()

    def toi(buf):
        return api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))

    def siblings(leaves, index):
        levels = mimc7.tree_build(leaves + [0] * ((1 << depth) - len(leaves)))
        return [levels[l][(index >> l) ^ 1] for l in range(depth)], levels[-1][0]

    token, chain_id = rnd.randrange(1 << 160), 1387
    note = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=10)
    pay = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=3)          # the payee's opening of c_pay
    rest = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=7)         # the payer's opening of c_change
    leaves = [rnd.randrange(R), withdraw_spec.leaf_of(note["nullifier"], note["secret"], note["amount"], token), rnd.randrange(R)]
    frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(tob(leaves)))
    sib, root_py = siblings(leaves, 1)
    assert toi(root) == [root_py]
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    # the transfer: 3 of the 10 to the payee, 7 back
    t_in = dict(note, index=1, siblings=sib, token=token, chain_id=chain_id, pay_commitment=mimc7.hash2(pay["nullifier"], pay["secret"]),
                pay_amount=pay["amount"], change_commitment=mimc7.hash2(rest["nullifier"], rest["secret"]))
    _b, vk, pk, close = _key(ctx, depth)
    proof, pub = circuit.transfer_prove(ctx, pk, depth, ctx.to_device(_pack(circuit, t_in)[None]), rs, return_public=True)
    t_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), t_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert t_pub[0] == root_py and t_pub[3:] == list(spec.leaves_of(t_in["pay_commitment"], 3, t_in["change_commitment"], 7, token))
    spent = withdraw_spec.build(depth, note["nullifier"], note["secret"], note["amount"], 9, 1, sib, token=token, chain_id=chain_id)[3]
    assert t_pub[1] == spent[2] == mimc7.hash2(note["nullifier"], 0), "the nullifier hash `withdraw` would publish for the same note"
    # the ledger appends pay_leaf, then change_leaf
    frontier, root = ctx.mimc7_append(depth, frontier, len(leaves), ctx.to_device(np.ascontiguousarray(pub[0, 3:5])))
    leaves += t_pub[3:]
    sib_pay, root_py = siblings(leaves, 3)
    sib_rest, _r = siblings(leaves, 4)
    assert toi(root) == [root_py]
    # the payee withdraws the pay note whole
    _b, vk, pk, close = _key(ctx, depth, "withdraw")
    rec = circuit.pack_inputs(pay["nullifier"], pay["secret"], pay["amount"], 9, 0, 3, sib_pay, token=token, chain_id=chain_id)
    proof, pub = circuit.prove_from_inputs(ctx, pk, depth, ctx.to_device(rec[None]), rs, return_public=True)
    w_pub = api.bytes_to_ints(pub[0])
    assert w_pub[0] == root_py and w_pub[3] == 3
    assert g16.verify(g16.vk_to_bytes(vk), w_pub, proof[0].tobytes(), lib=lib) is True
    close()
    # the payer takes 2 of the change note out and keeps 5
    _b, vk, pk, close = _key(ctx, depth, "split")
    s_in = dict(rest, recipient=9, amount_out=2, index=4, siblings=sib_rest, token=token, chain_id=chain_id, change_commitment=rnd.randrange(R))
    proof, pub = circuit.split_prove(ctx, pk, depth, ctx.to_device(circuit.pack_split_inputs(**s_in)[None]), rs, return_public=True)
    s_pub = api.bytes_to_ints(pub[0])
    assert s_pub == split_spec.build(depth, **s_in)[3][1:8] and s_pub[0] == root_py
    assert g16.verify(g16.vk_to_bytes(vk), s_pub, proof[0].tobytes(), lib=lib) is True
    close()
