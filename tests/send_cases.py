"""Send- and redeem-statement cases shared by the CPU-interpreter run and the GPU run.  The two statements have one front (claim's)
and differ in their back (transfer's, split's), so every case is written once over a small description of the statement -- SEND here,
REDEEM in tests/redeem_cases.py, which binds the same functions: the product's two R1CS builders and the HIP witness kernel against
the plain restatement (tests/send_spec.py, tests/redeem_spec.py), then proofs -- byte-identical to the C restatement's, accepted for
the public inputs and refused for anything else --, five forged witnesses that must stay unprovable, the one nullifier hash of the
three owned statements, the theft the owned form exists to stop, the boundary check of the records, the slab loop past its first
slab, and two hops through the pool with no claim between them."""
import functools
import random
import types

import numpy as np
import pytest

from oracle.py import babyjubjub as bj
from oracle.py import fields, mimc7
from tests import claim_spec
from tests import send_spec
from tests import view_note_spec
from tests.claim_cases import _siblings, _tob
from tests.transfer_cases import _check_witness, _failing, _wit_bytes
from tests.withdraw_cases import _rows, _oracle_rows

R = fields.R
ELL = claim_spec.ELL
TOP = (1 << 128) - 1
_TOXIC = (45, 46, 47, 48, 49)
N_EDGES = 7
# name: the statement's; part: the record's field that is paid (the rest is the change); extra: the fields only this statement has;
# wrong_key: a statement with the same n_pub and another wire count; leaf_forge / token_forge: the spec's forge keys of the output leaf
# (gadget 5 + depth, public wire leaf_wire) and of its asset (gadget 4 + depth)
SEND = types.SimpleNamespace(
    name="send", spec=send_spec, n_pub=5, part="pay_amount", part_wire=10, change_wire=12, leaf_wire=4, leaf_commitment="pay_commitment",
    fields=("x", "amount", "token", "chain_id", "pay_commitment", "pay_amount", "change_commitment", "index"),
    extra=("pay_commitment",), wrong_key="transfer", leaf_forge="pay_leaf", token_forge="pay_asset_token")


def _inputs(st, rnd, depth, **values):
    amount = rnd.randrange(1, 1 << 64)
    i = dict(x=rnd.randrange(ELL), amount=amount, index=rnd.randrange(1 << depth), siblings=[rnd.randrange(R) for _ in range(depth)],
             token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32), change_commitment=rnd.randrange(R))
    i[st.part] = rnd.randrange(amount + 1)
    for name in st.extra:
        i[name] = rnd.randrange(R)
    i.update(values)
    return i


def edge_inputs(st, rnd, depth, n):
    """n requests of which the first seven (as many as n has) carry, by construction: x = 0 (P is the identity: every partial sum is
    (0, 1)) at index 0, the all-left walk; x = 1 at the last leaf, the all-right walk; x = l - 1, the largest key, with amount = part =
    2^128 - 1 (change 0) and the commitments, the token and whatever else the statement has = r - 1; an x with bit 250 set (the last
    step of the multiplication adds; in redeem with amount_out = amount); part = 0 (everything into change); amount = 0; a random
    split"""
    ins = [_inputs(st, rnd, depth) for _ in range(max(n, N_EDGES))]
    ins[0].update(x=0, index=0)
    ins[1].update(x=1, index=(1 << depth) - 1)
    ins[2].update({st.part: TOP, **{name: R - 1 for name in st.extra}}, x=ELL - 1, amount=TOP, change_commitment=R - 1, token=R - 1)
    if st.name == "redeem":
        ins[2].update(chain_id=R - 1)
    ins[3].update(x=(1 << 250) | rnd.randrange(ELL - (1 << 250)))
    if st.name == "redeem":
        ins[3].update(amount_out=ins[3]["amount"])
    ins[4].update({st.part: 0})
    ins[5].update({st.part: 0}, amount=0)
    ins[6].update({st.part: rnd.randrange(1, 1 << 63)}, amount=rnd.randrange(1 << 63, 1 << 64))
    assert ins[3]["x"] < ELL and ins[3]["x"] >> 250 == 1 and 0 < ins[6][st.part] < ins[6]["amount"]
    return ins[:n]


def _pack(st, circuit, i):
    return getattr(circuit, f"pack_{st.name}_inputs")(**i)


def _spec(st, i, depth, forge=None):
    return st.spec.build(depth, forge=forge, **i)


def _witness(st, circuit, ctx, depth, recs_d):
    return getattr(circuit, st.name + "_witness")(ctx, depth, recs_d)


def _prove(st, circuit, ctx, pk, depth, recs_d, rs, **kw):
    return getattr(circuit, st.name + "_prove")(ctx, pk, depth, recs_d, rs, **kw)


def _key(st, ctx, depth, statement=None):
    """(key blob, vk, loaded key, close) of the statement (or of another one) at `depth`; on the CPU interpreter the cases of a session
    share one key per shape and `close` does nothing (as tests/claim_cases._key)"""
    from owshen_amd import circuit, groth16 as g16
    statement = statement or st.name
    shared = type(ctx).__module__ == "tests.emu"
    cache = ctx.__dict__.setdefault("_owned_spend_keys", {}) if shared else {}
    k = (statement, depth)
    if k not in cache:
        r1 = getattr(circuit, statement + "_r1cs")(ctx.mimc7_constants(), depth)
        blob, vk = g16.setup(ctx, r1, *_TOXIC)
        cache[k] = (blob, vk, g16.ProvingKey(ctx, blob))
    blob, vk, pk = cache[k]
    return blob, vk, pk, (lambda: None) if shared else pk.close


def _publics(st, i, depth):
    """the public inputs of request i, from the oracle's primitives alone"""
    p = bj.multiply(bj.BASE, i["x"])
    root = mimc7.merkle_root_from_path(mimc7.hash2(mimc7.hash2(*p), mimc7.hash2(i["amount"], i["token"])), i["index"], i["siblings"])[-1]
    change_leaf = mimc7.hash2(i["change_commitment"], mimc7.hash2(i["amount"] - i[st.part], i["token"]))
    if st.name == "send":
        pay_leaf = mimc7.hash2(i["pay_commitment"], mimc7.hash2(i["pay_amount"], i["token"]))
        return [root, mimc7.hash2(i["x"], 1), i["chain_id"], pay_leaf, change_leaf]
    return [root, mimc7.hash2(i["x"], 1), i["recipient"], i["amount_out"], i["token"], i["chain_id"], change_leaf]


def case_r1cs_and_witness_match_spec(st, ctx, depth, n, seed=1):
    """both builders give the spec's rows (A, B and C with the identity rows, on request 0), og_*_shape is the spec's shape, and the
    kernel's witnesses are the spec's z integer for integer at requests 0..6, 63, 64 and n - 1 of a call of n requests"""
    import ctypes as C
    from owshen_amd import api, circuit
    spec = st.spec
    rnd = random.Random(seed * 1000 + depth)
    ins = edge_inputs(st, rnd, depth, n)
    shp = (C.c_uint64 * 3)()
    ctx._check(getattr(ctx._lib, f"og_{st.name}_shape")(depth, shp))
    assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == getattr(circuit, st.name + "_shape")(depth)
    assert int(shp[2]) == spec.N_PUB == st.n_pub
    r1 = getattr(circuit, st.name + "_r1cs")(ctx.mimc7_constants(), depth)
    nat = getattr(circuit, st.name + "_r1cs_native")(ctx, depth)
    assert (nat.n_wires, nat.n_pub, nat.n_constraints, nat.log_d) == (r1.n_wires, r1.n_pub, r1.n_constraints, r1.log_d)
    assert (r1.n_wires, r1.n_constraints) == spec.shape(depth) and r1.n_pub == st.n_pub
    wit = ctx.to_host(_witness(st, circuit, ctx, depth, ctx.to_device(np.stack([_pack(st, circuit, i) for i in ins]))))
    checked = sorted((set(range(N_EDGES)) | {63, 64, n - 1}) & set(range(n)))   # the edges, both sides of a wave's end, the last lane
    for k in checked:
        i = ins[k]
        m, l, cons, z = _spec(st, i, depth)
        assert (m, l) == (r1.n_wires, r1.n_pub) and len(cons) == r1.n_constraints
        _check_witness(api, wit[k], z, f"{st.name} witness {k}")
        assert z[1:1 + st.n_pub] == _publics(st, i, depth)
        assert z[st.part_wire] == i[st.part] and z[st.change_wire] == i["amount"] - i[st.part]
        if k == 0:
            ident, empty = [[(w, 1)] for w in range(l + 1)], [[] for _ in range(l + 1)]
            for name, which, extra in (("a", 0, ident), ("b", 1, empty), ("c", 2, empty)):
                assert _rows(getattr(r1, name)) == _oracle_rows(cons, which, extra), name
                assert _rows(getattr(nat, name)) == _rows(getattr(r1, name)), name
    # the ledger's side: the leaves through og_mimc7_hash2_d
    i = ins[min(2, n - 1)]
    pub = _publics(st, i, depth)
    if st.name == "send":
        assert circuit.send_leaves(i["pay_commitment"], i["pay_amount"], i["change_commitment"], i["amount"] - i["pay_amount"], i["token"],
                                   ctx) == (pub[3], pub[4])
    else:
        assert circuit.redeem_change_leaf(i["change_commitment"], i["amount"] - i["amount_out"], i["token"], ctx) == pub[6]


def case_end_to_end(st, ctx, depth, n=4, seed=2, key=None):
    """records -> proofs: the C restatement's bytes, the generic prover's bytes from the generated witnesses; public_out is wires
    1..n_pub, with and without it the same proofs; og_verify and og_verify_batch_d (under og_vk_load) accept; refused with any one
    input changed by one and with a neighbour's inputs"""
    from oracle.c import binding as oc
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(st, ctx, depth)
    ins = edge_inputs(st, rnd, depth, N_EDGES)[:n]
    recs = np.stack([_pack(st, circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    proofs, pub = _prove(st, circuit, ctx, pk, depth, ctx.to_device(recs), rs, return_public=True)
    wit_d = _witness(st, circuit, ctx, depth, ctx.to_device(recs))
    wit = ctx.to_host(wit_d)
    assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:1 + st.n_pub]).tobytes()
    assert _prove(st, circuit, ctx, pk, depth, ctx.to_device(recs), rs).tobytes() == proofs.tobytes()    # public_out = NULL
    assert pk.prove_batch_device(wit_d, rs).tobytes() == proofs.tobytes()                               # the generic entry point
    ck = oc.prepared_key_from_blob(blob)
    vkb = g16.vk_to_bytes(vk)
    lib = ctx._lib
    for t, i in enumerate(ins):
        assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"{st.name} proof {t} differs from the C restatement"
        good = api.bytes_to_ints(pub[t])
        assert good == _publics(st, i, depth)
        p = proofs[t].tobytes()
        assert g16.verify(vkb, good, p, lib=lib) is True
        for slot in range(st.n_pub):          # every public input + 1
            forged = list(good)
            forged[slot] = (forged[slot] + 1) % R
            assert g16.verify(vkb, forged, p, lib=lib) is False, slot
    if n > 1:
        assert g16.verify(vkb, pub[1], proofs[0].tobytes(), lib=lib) is False
    with g16.VerifyingKey(ctx, vkb) as dvk:
        assert dvk.n_pub == st.n_pub
        assert dvk.verify_batch(pub, proofs).all()
        if n > 1:
            assert not dvk.verify_batch(np.roll(pub, 1, axis=0), proofs).any()       # every proof against a neighbour's inputs
    close()


def case_batch_130_verifies(st, ctx, depth, key, n=130):
    """n requests in one prove call: all accepted by og_verify_batch_d under an og_vk_load of the key, proof 0 against proof 1's inputs
    refused, proofs 0, 64 and n - 1 byte-identical to the C restatement"""
    from oracle.c import binding as oc
    from owshen_amd import circuit, groth16 as g16
    blob, vk, pk, _close = key
    rnd = random.Random(130)
    ins = edge_inputs(st, rnd, depth, n)
    recs = np.stack([_pack(st, circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    recs_d = ctx.to_device(recs)
    proofs, pub = _prove(st, circuit, ctx, pk, depth, recs_d, rs, return_public=True)
    with g16.VerifyingKey(ctx, g16.vk_to_bytes(vk)) as dvk:
        assert dvk.n_pub == st.n_pub
        ok = dvk.verify_batch(pub, proofs)
        assert ok.all(), f"{int((~ok).sum())} of {n} {st.name} proofs refused"
        assert not dvk.verify_batch(pub[1:2], proofs[0:1])[0]
    idx = [0, 64, n - 1]
    wit = ctx.to_host(_witness(st, circuit, ctx, depth, recs_d[idx]))
    ck = oc.prepared_key_from_blob(blob)
    for j, t in enumerate(idx):
        assert proofs[t].tobytes() == ck.prove(wit[j], *rs[t]), t


def forgeries(st, rnd, depth):
    """(honest request, [(name, z, the rows that must fail)]): five witnesses that are wrong in one place each, every other wire what
    an honest prover's would be (the spec's build(forge=...)).
    the second key: the bits, the wire x and the nullifier hash of x + l for an x < 2^251 - l (asserted), so the recomposition holds,
      P = (x + l) BASE is the note's key and the root is the tree's -- only the comparison fails: at every 0-bit of l - 1 under a
      1-bit of x + l for as long as t stays 1;
    a bit wire of x equal to 2: bit 0 of an x = 2 (mod 4) becomes 2 and bit 1 gives way, so the recomposition still holds, and every
      wire of the multiplication follows the rows with b = 2 -- only the booleanity row of bit 0 in the multiplication fails;
    an overdraw: part = amount + 1 and change = r - 1 = -1, so the sum holds in the field; the bit wires are the low 128 bits and the
      output gadgets follow -- only the recomposition of `change`, the last of its range rows, fails;
    an output leaf for another amount: the leaf's public wire = H(commitment, H(its amount + 1, token)) over honest gadgets -- only
      the output row of that gadget fails;
    another token in the output asset: the gadget's values are those of H(., token + 1) and the leaf follows, but its rows name the
      ONE token wire -- the two rows of the second permutation's first round that read the right input, and the output row, fail"""
    spec = st.spec
    seed_x = rnd.randrange((1 << 251) - ELL)
    assert seed_x < (1 << 251) - ELL
    honest = _inputs(st, rnd, depth, x=seed_x)
    m, _l, cons, _z = _spec(st, honest, depth)
    second = seed_x + ELL
    assert second < (1 << 251)
    z = _spec(st, honest, depth, forge={"bits": [(second >> i) & 1 for i in range(spec.N_BITS)], "x": second})[3]
    rows, t = [], 1                 # the comparison, walked here: a 0-bit of l - 1 under a 1-bit of x + l fails while t is still 1
    for i in reversed(range(spec.N_BITS)):
        b = (second >> i) & 1
        if (claim_spec.M >> i) & 1:
            t &= b
        elif b and t:
            rows.append(spec.ROW_CMP + (spec.N_BITS - 1 - i))
    assert rows and all(spec.ROW_CMP <= r < spec.ROW_MUL for r in rows)
    out = [("the second key x + l", z, rows)]
    even = dict(honest, x=(rnd.randrange(ELL >> 2) << 2) | 2)
    bits = [(even["x"] >> i) & 1 for i in range(spec.N_BITS)]
    bits[0], bits[1] = 2, 0
    out.append(("a bit wire of x equal to 2", _spec(st, even, depth, forge={"bits": bits})[3], [spec.ROW_MUL]))
    wrapped = dict(honest, **{st.part: honest["amount"] + 1})
    z = _spec(st, wrapped, depth, forge={})[3]
    assert z[st.part_wire] == honest["amount"] + 1 and z[st.change_wire] == R - 1
    w = spec.first_range_wire(depth) + 128
    assert z[w:w + 128] == [((R - 1) >> k) & 1 for k in range(128)], "the bit wires of change are its low 128 bits"
    out.append(("an overdraw", z, [spec.ROW_CHANGE_RANGE]))
    leaf_amount = honest[st.part] if st.name == "send" else honest["amount"] - honest[st.part]
    other = mimc7.hash2(honest[st.leaf_commitment], mimc7.hash2(leaf_amount + 1, honest["token"]))
    out.append(("an output leaf for another amount", _spec(st, honest, depth, forge={st.leaf_forge: other})[3],
                [spec.gadget_row(depth, 5 + depth) + 729]))
    g = spec.gadget_row(depth, 4 + depth)
    out.append(("another token in the output asset", _spec(st, honest, depth, forge={st.token_forge: honest["token"] + 1})[3],
                [g + 365, g + 368, g + 729]))
    for name, z, rows in out:
        assert len(z) == m and _failing(cons, z) == rows, (name, _failing(cons, z), rows)
    return honest, out


def case_forgeries_are_unprovable(st, ctx, depth, seed=3, key=None):
    """each forged witness fails exactly its rows on the CPU, and og_prove_batch_d answers OG_ERR_UNSATISFIED for it; the honest
    witness proves"""
    from owshen_amd import api
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(st, ctx, depth)
    honest, forged = forgeries(st, rnd, depth)
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    for name, z, _rows_failing in forged:
        with pytest.raises(api.OwshenGpuError) as e:
            pk.prove_batch_device(ctx.to_device(_wit_bytes(z)), rs)
        assert e.value.code == -4, (name, str(e.value))
    assert pk.prove_batch_device(ctx.to_device(_wit_bytes(_spec(st, honest, depth)[3])), rs).shape == (1, 256)
    close()


def case_one_spent_set(ctx, depth=2, seed=8):
    """for the same owned note, wire 2 of a claim, a send and a redeem witness is the one value H(x, 1): whichever statement spends
    the note, the ledger's spent set sees the same nullifier hash"""
    from owshen_amd import api, circuit
    from tests.redeem_cases import REDEEM
    rnd = random.Random(seed)
    for x in (rnd.randrange(ELL), 0, ELL - 1):
        common = dict(x=x, amount=rnd.randrange(1, 1 << 64), index=rnd.randrange(1 << depth), siblings=[rnd.randrange(R) for _ in range(depth)],
                      token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32))
        claim = circuit.pack_claim_inputs(out_commitment=rnd.randrange(R), **common)
        send = _pack(SEND, circuit, dict(common, pay_commitment=rnd.randrange(R), pay_amount=1, change_commitment=rnd.randrange(R)))
        redeem = _pack(REDEEM, circuit, dict(common, recipient=rnd.randrange(1 << 160), amount_out=1, change_commitment=rnd.randrange(R)))
        got = []
        for name, rec in (("claim", claim), ("send", send), ("redeem", redeem)):
            wit = ctx.to_host(getattr(circuit, name + "_witness")(ctx, depth, ctx.to_device(rec[None])))
            got.append(api.bytes_to_ints(wit[0, 1:3]))
        want = mimc7.hash2(x, 1)
        assert [g[1] for g in got] == [want] * 3, (x, got)
        assert got[0][0] == got[1][0] == got[2][0], "the three statements publish one root for the note"


def case_the_theft_is_closed(st, ctx, depth=2, seed=5):
    """tests/claim_cases.case_the_theft_is_closed for this statement: an owned note is sealed and its leaf appended.  A record built
    from everything the sender knows -- its best x' is t mod l, the only scalar it holds -- publishes a root that is not the tree's;
    the payee's record publishes the tree's root"""
    from owshen_amd import api, circuit
    from tests import owned_note_spec as note_spec
    rnd = random.Random(seed)
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))
    sk = rnd.randrange(1, R)
    pk = bj.multiply(bj.BASE, sk)
    e, amount, token = rnd.randrange(1, R), 12, rnd.randrange(1 << 160)
    memos_d, notes_d, ok = ctx.note_seal_owned(ctx.to_device(_tob([e, *pk, amount, token]).reshape(1, 5, 32)))
    assert ok.tolist() == [1]
    c, leaf = toi(notes_d)
    leaves = [rnd.randrange(R), leaf]
    _frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(_tob(leaves)))
    sib, root_py = _siblings(depth, leaves, 1)
    assert toi(root) == [root_py]
    s = bj.multiply(pk, e)          # everything the sender knows
    _tag, t, _pa, _pt = note_spec.kdf(s)
    p = note_spec.one_time_key(pk, t)
    assert mimc7.hash2(*p) == c, "the sender can compute P and c"
    common = _inputs(st, rnd, depth, amount=amount, index=1, siblings=sib, token=token, chain_id=1, **{st.part: 5})
    thief = dict(common, x=t % ELL)
    payee = dict(common, x=(sk + t) % ELL)
    assert bj.multiply(bj.BASE, thief["x"]) != p and bj.multiply(bj.BASE, payee["x"]) == p
    wit = ctx.to_host(_witness(st, circuit, ctx, depth, ctx.to_device(np.stack([_pack(st, circuit, thief), _pack(st, circuit, payee)]))))
    pub_thief, pub_payee = api.bytes_to_ints(wit[0, 1:1 + st.n_pub]), api.bytes_to_ints(wit[1, 1:1 + st.n_pub])
    assert pub_thief[0] != root_py, "the sender's record publishes the tree's root"
    assert pub_payee[0] == root_py and pub_payee[1] == mimc7.hash2(payee["x"], 1)
    assert pub_thief == _spec(st, thief, depth)[3][1:1 + st.n_pub] and pub_payee == _spec(st, payee, depth)[3][1:1 + st.n_pub]


def case_record_boundary(st, ctx, depth, seed=4, key=None, other_keys=True):
    """one bad record per case: OG_ERR_INVALID names the record and its lowest offending field, from the witness call and from the
    prove call; x = l is refused and x = l - 1 taken; the largest well-formed record passes; a key of the wrong statement is refused"""
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(st, ctx, depth)
    nrec = 4
    fields_ = st.fields
    ins = [_inputs(st, rnd, depth) for _ in range(nrec)]
    good = np.stack([_pack(st, circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    part, f_part, f_index = st.part, st.fields.index(st.part), st.fields.index("index")
    assert f_index == 7 and f_part == (5 if st.name == "send" else 3)

    def le(v):
        return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)

    def with_fields(rec, **fv):
        """s<l>: sibling l"""
        x = good.copy()
        for name, value in fv.items():
            x[rec, fields_.index(name) if name in fields_ else len(fields_) + int(name[1:])] = le(value)
        return x

    bad_cases = [(with_fields(f % nrec, **{name: R}), f % nrec, f, name) for f, name in enumerate(fields_)]
    bad_cases += [(with_fields(1, **{f"s{l}": R}), 1, len(fields_) + l, f"sibling {l}") for l in range(depth)]
    bad_cases += [
        (with_fields(2, x=ELL), 2, 0, "x"),
        (with_fields(0, x=ELL + 1), 0, 0, "x"),
        (with_fields(1, x=1 << 251), 1, 0, "x"),
        (with_fields(1, amount=1 << 128, **{part: 0}), 1, 1, "amount"),
        (with_fields(0, amount=TOP, **{part: 1 << 128}), 0, f_part, part),
        (with_fields(2, **{part: ins[2]["amount"] + 1}), 2, f_part, part),                     # an overdraw
        (with_fields(3, amount=1 << 64, **{part: (1 << 64) + 1}), 3, f_part, part),           # (decided above the low word)
        (with_fields(3, index=1 << depth), 3, f_index, "index"),
        (with_fields(2, amount=1 << 128, x=ELL, change_commitment=R), 2, 0, "x"),             # three fields offend: the lowest is named
        (with_fields(1, index=1 << depth, **{part: ins[1]["amount"] + 1}), 1, f_part, part),
        (with_fields(3, index=1 << depth, **{f"s{depth - 1}": R}), 3, f_index, "index"),
    ]
    for k, (packed, rec, field, name) in enumerate(bad_cases):
        for call in (lambda d: _witness(st, circuit, ctx, depth, d), lambda d: _prove(st, circuit, ctx, pk, depth, d, rs)):
            with pytest.raises(api.OwshenGpuError) as e:
                call(ctx.to_device(packed))
            assert e.value.code == -1 and f"og_{st.name}" in str(e.value), (k, str(e.value))
            assert f"input record {rec}: field {field} ({name})" in str(e.value), (k, str(e.value))
    largest = {name: R - 1 for name in fields_ if name not in ("x", "amount", part, "index")}
    edge = with_fields(0, x=ELL - 1, amount=TOP, index=(1 << depth) - 1, **{part: TOP, f"s{depth - 1}": R - 1}, **largest)
    _witness(st, circuit, ctx, depth, ctx.to_device(edge))
    if other_keys:
        from tests import transfer_cases
        _b, _v, other, close_other = transfer_cases._key(ctx, depth, st.wrong_key)
        assert other.n_pub == st.n_pub
        with pytest.raises(api.OwshenGpuError) as e:
            _prove(st, circuit, ctx, other, depth, ctx.to_device(good), rs)
        assert e.value.code == -1 and f"not for this {st.name}-statement shape" in str(e.value), str(e.value)
        close_other()
    close()


def case_second_slab(st, ctx, depth=2, seed=7):
    """the slab loop past its first slab (tests/statement_slab_cases.py, for this statement): OG_SLAB_MAX = 2 makes three slabs of five
    requests; the profiler counts three witness launches, proofs and public outputs are those of the one-slab call, and a malformed
    record 3 is named by its index in the call.  `ctx` reads the hooks."""
    from owshen_amd import api, circuit
    from tests.statement_slab_cases import _env
    rnd = random.Random(seed)
    blob, vk, pk, close = _key(st, ctx, depth)
    recs = np.stack([_pack(st, circuit, i) for i in edge_inputs(st, rnd, depth, 5)])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(5)]

    def witness_calls(call):
        ctx.profile(True)
        try:
            out = call()
            return out, ctx.profile_read()["witness"][1]
        finally:
            ctx.profile(False)

    (proofs, pub), slabs = witness_calls(lambda: _prove(st, circuit, ctx, pk, depth, ctx.to_device(recs), rs, return_public=True))
    assert slabs == 1
    with _env(OG_SLAB_MAX="2"):
        (p2, pub2), slabs = witness_calls(lambda: _prove(st, circuit, ctx, pk, depth, ctx.to_device(recs), rs, return_public=True))
        assert slabs == 3, f"OG_SLAB_MAX=2 gave {slabs} slabs for 5 requests, not 3"
        assert p2.tobytes() == proofs.tobytes() and pub2.tobytes() == pub.tobytes()
        bad = recs.copy()
        bad[3, 0] = np.frombuffer(ELL.to_bytes(32, "little"), dtype=np.uint8)
        with pytest.raises(api.OwshenGpuError) as e:
            _prove(st, circuit, ctx, pk, depth, ctx.to_device(bad), rs)
        assert e.value.code == -1 and "input record 3: field 0 (x)" in str(e.value), str(e.value)
    close()


def case_two_hops_with_no_claim(ctx, depth=3, seed=9):
    """a note is sealed to wallet A's view address and appended; A finds it with (v, PS), unlocks x and `send`s: the pay note sealed to
    wallet B's view address, the change note to its own, both commitments the c the seals returned -- the published leaves are the
    seals' leaves byte for byte.  The ledger appends both; B finds and unlocks the pay note and `redeem`s part of it to a recipient
    under the new root; A `claim`s its change note, so the existing statement still works beside the new ones.  Three proofs, none
    of them a claim in front of a spend."""
    from owshen_amd import api, circuit, groth16 as g16
    from tests import claim_cases
    from tests.redeem_cases import REDEEM
    rnd = random.Random(seed)
    lib = ctx._lib
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))

    class Wallet:
        def __init__(self):
            self.v, self.sk = rnd.randrange(1, ELL), rnd.randrange(1, ELL)
            self.pv, self.ps = bj.multiply(bj.BASE, self.v), bj.multiply(bj.BASE, self.sk)

        def seal(self, amount, token):
            """a note for this wallet: (memo, c, leaf)"""
            req = _tob([rnd.randrange(1, R), *self.pv, *self.ps, amount, token]).reshape(1, 7, 32)
            memos_d, notes_d, ok = ctx.note_seal_view(ctx.to_device(req))
            assert ok.tolist() == [1]
            c, leaf = toi(notes_d)
            return memos_d, c, leaf

        def find(self, memos_d, leaf):
            """scan with (v, PS), unlock with sk: x, amount, token"""
            leaf_d = ctx.to_device(_tob([leaf]))
            rows_d, hit = ctx.note_scan_view(self.v, self.ps, memos_d, leaf_d)
            assert hit.tolist() == [1]
            t, amount, token, c = toi(rows_d)
            assert view_note_spec.scan_view(self.v, self.ps, tuple(toi(memos_d)), leaf) == (1, (t, amount, token, c))
            unlocked_d, ok = ctx.note_unlock(self.sk, rows_d, leaf_d)
            assert ok.tolist() == [1]
            x, amount, token, c = toi(unlocked_d)
            assert x == (self.sk + t) % ELL and mimc7.hash2(*bj.multiply(bj.BASE, x)) == c
            return x, amount, token

    a, b = Wallet(), Wallet()
    token, chain_id, amount, pay_amount, amount_out = rnd.randrange(1 << 160), 1387, 100, 60, 25
    memo_a, _c_a, leaf_a = a.seal(amount, token)
    leaves = [rnd.randrange(R), leaf_a]
    frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(_tob(leaves)))
    sib, root_py = _siblings(depth, leaves, 1)
    assert toi(root) == [root_py]
    assert ctx.note_scan_view(b.v, b.ps, memo_a, ctx.to_device(_tob([leaf_a])))[1].tolist() == [0], "B sees A's note"
    x_a, got_amount, got_token = a.find(memo_a, leaf_a)
    assert (got_amount, got_token) == (amount, token)
    # hop 1: A sends pay_amount to B and keeps the change, both as view notes
    memo_pay, c_pay, leaf_pay = b.seal(pay_amount, token)
    memo_chg, c_chg, leaf_chg = a.seal(amount - pay_amount, token)
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    rec = dict(x=x_a, amount=amount, index=1, siblings=sib, token=token, chain_id=chain_id, pay_commitment=c_pay, pay_amount=pay_amount,
               change_commitment=c_chg)
    _b, vk, pk_s, close = _key(SEND, ctx, depth)
    proof, pub = circuit.send_prove(ctx, pk_s, depth, ctx.to_device(_pack(SEND, circuit, rec)[None]), rs, return_public=True)
    s_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), s_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert s_pub == [root_py, mimc7.hash2(x_a, 1), chain_id, leaf_pay, leaf_chg]
    assert pub[0, 3:5].tobytes() == _tob([leaf_pay, leaf_chg]).tobytes(), "the published leaves are the leaves the seals returned"
    frontier, root = ctx.mimc7_append(depth, frontier, len(leaves), ctx.to_device(np.ascontiguousarray(pub[0, 3:5])))
    leaves += [leaf_pay, leaf_chg]
    sib_pay, root_py = _siblings(depth, leaves, 2)
    assert toi(root) == [root_py]
    # hop 2: B finds the pay note and redeems part of it
    x_b, got_amount, got_token = b.find(memo_pay, leaf_pay)
    assert (got_amount, got_token) == (pay_amount, token) and x_b != x_a
    recipient, c_rest = rnd.randrange(1 << 160), rnd.randrange(R)
    rec = dict(x=x_b, amount=pay_amount, recipient=recipient, amount_out=amount_out, index=2, siblings=sib_pay, token=token, chain_id=chain_id,
               change_commitment=c_rest)
    _b, vk, pk_r, close = _key(REDEEM, ctx, depth)
    proof, pub = circuit.redeem_prove(ctx, pk_r, depth, ctx.to_device(_pack(REDEEM, circuit, rec)[None]), rs, return_public=True)
    r_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), r_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert r_pub == [root_py, mimc7.hash2(x_b, 1), recipient, amount_out, token, chain_id,
                     mimc7.hash2(c_rest, mimc7.hash2(pay_amount - amount_out, token))]
    # A claims its change note: the existing statement beside the new ones
    x_c, got_amount, got_token = a.find(memo_chg, leaf_chg)
    assert (got_amount, got_token) == (amount - pay_amount, token)
    sib_chg, _root = _siblings(depth, leaves, 3)
    out_commitment = rnd.randrange(R)
    rec = dict(x=x_c, amount=amount - pay_amount, index=3, siblings=sib_chg, token=token, chain_id=chain_id, out_commitment=out_commitment)
    _b, vk, pk_c, close = claim_cases._key(ctx, depth)
    proof, pub = circuit.claim_prove(ctx, pk_c, depth, ctx.to_device(circuit.pack_claim_inputs(**rec)[None]), rs, return_public=True)
    c_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), c_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert c_pub == [root_py, mimc7.hash2(x_c, 1), chain_id, mimc7.hash2(out_commitment, mimc7.hash2(amount - pay_amount, token))]
    assert len({s_pub[1], r_pub[1], c_pub[1]}) == 3


# the cases of this statement
case_send_r1cs_and_witness_match_spec = functools.partial(case_r1cs_and_witness_match_spec, SEND)
case_send_end_to_end = functools.partial(case_end_to_end, SEND)
case_send_batch_130_verifies = functools.partial(case_batch_130_verifies, SEND)
case_send_forgeries_are_unprovable = functools.partial(case_forgeries_are_unprovable, SEND)
case_send_the_theft_is_closed = functools.partial(case_the_theft_is_closed, SEND)
case_send_record_boundary = functools.partial(case_record_boundary, SEND)
case_send_second_slab = functools.partial(case_second_slab, SEND)
key = functools.partial(_key, SEND)
