"""Claim-statement cases shared by the CPU-interpreter run and the GPU run: the product's two R1CS builders and the HIP witness kernel
against the plain restatement in tests/claim_spec.py, then proofs -- byte-identical to the C restatement's, accepted for the four
public inputs and refused for anything else --, four forged witnesses that must stay unprovable, the theft the statement exists to
stop, the boundary check of the records, the slab loop past its first slab, and an owned note through the pool."""
import random

import numpy as np
import pytest

from oracle.py import babyjubjub as bj
from oracle.py import fields, mimc7, withdraw as withdraw_spec
from tests import claim_spec as spec
from tests import owned_note_spec as note_spec
from tests.transfer_cases import _check_witness, _failing, _wit_bytes
from tests.withdraw_cases import _rows, _oracle_rows

R = fields.R
ELL = spec.ELL
TOP = (1 << 128) - 1
_TOXIC = (35, 36, 37, 38, 39)
FIELDS = ("x", "amount", "token", "chain_id", "out_commitment", "index")


def _inputs(rnd, depth, **values):
    i = dict(x=rnd.randrange(ELL), amount=rnd.randrange(1, 1 << 64), index=rnd.randrange(1 << depth),
             siblings=[rnd.randrange(R) for _ in range(depth)], token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32),
             out_commitment=rnd.randrange(R))
    i.update(values)
    return i


def edge_inputs(rnd, depth, n):
    """n >= 5 requests; the first five carry, by construction: x = 0 (P is the identity: every partial sum is (0, 1)) at index 0, the
    all-left walk; x = 1 at the last leaf, the all-right walk; x = l - 1, the largest key, with amount = 2^128 - 1 and
    out_commitment = token = r - 1; an x with bit 250 set (the last step of the multiplication adds); a random x with amount = 0"""
    assert n >= 5
    ins = [_inputs(rnd, depth) for _ in range(n)]
    ins[0].update(x=0, index=0)
    ins[1].update(x=1, index=(1 << depth) - 1)
    ins[2].update(x=ELL - 1, amount=TOP, out_commitment=R - 1, token=R - 1)
    ins[3].update(x=(1 << 250) | rnd.randrange(ELL - (1 << 250)))
    ins[4].update(amount=0)
    assert ins[3]["x"] < ELL and ins[3]["x"] >> 250 == 1
    return ins


def _pack(circuit, i):
    return circuit.pack_claim_inputs(**i)


def _spec(i, depth, forge=None):
    return spec.build(depth, forge=forge, **i)


def _key(ctx, depth, statement="claim"):
    """(key blob, vk, loaded key, close) of the claim statement (or of another one) at `depth`; on the CPU interpreter the cases of a
    session share one key per shape and `close` does nothing (as tests/transfer_cases._key)"""
    from owshen_amd import circuit, groth16 as g16
    shared = type(ctx).__module__ == "tests.emu"
    cache = ctx.__dict__.setdefault("_claim_keys", {}) if shared else {}
    k = (statement, depth)
    if k not in cache:
        r1 = getattr(circuit, statement + "_r1cs")(ctx.mimc7_constants(), depth)
        blob, vk = g16.setup(ctx, r1, *_TOXIC)
        cache[k] = (blob, vk, g16.ProvingKey(ctx, blob))
    blob, vk, pk = cache[k]
    return blob, vk, pk, (lambda: None) if shared else pk.close


def case_r1cs_and_witness_match_spec(ctx, depth, n, seed=1):
    """both builders give the spec's rows, og_claim_shape is the spec's shape, and the kernel's witnesses are the spec's z integer for
    integer -- over the edge requests of `edge_inputs`, in a call of n requests"""
    import ctypes as C
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    ins = edge_inputs(rnd, depth, n)
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_claim_shape(depth, shp))
    assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.claim_shape(depth) and int(shp[2]) == spec.N_PUB == 4
    r1 = circuit.claim_r1cs(ctx.mimc7_constants(), depth)
    nat = circuit.claim_r1cs_native(ctx, depth)
    assert (nat.n_wires, nat.n_pub, nat.n_constraints, nat.log_d) == (r1.n_wires, r1.n_pub, r1.n_constraints, r1.log_d)
    assert (r1.n_wires, r1.n_constraints) == spec.shape(depth) and r1.n_pub == 4
    wit = ctx.to_host(circuit.claim_witness(ctx, depth, ctx.to_device(np.stack([_pack(circuit, i) for i in ins]))))
    checked = sorted(set(range(min(n, 6))) | {63, 64, n - 1} & set(range(n)))   # the edges, both sides of a wave's end, the last lane
    for k in checked:
        i = ins[k]
        m, l, cons, z = _spec(i, depth)
        assert (m, l) == (r1.n_wires, r1.n_pub) and len(cons) == r1.n_constraints
        _check_witness(api, wit[k], z, f"claim witness {k}")
        p = bj.multiply(bj.BASE, i["x"])
        c, asset = mimc7.hash2(*p), mimc7.hash2(i["amount"], i["token"])
        assert z[1] == mimc7.merkle_root_from_path(mimc7.hash2(c, asset), i["index"], i["siblings"])[-1] and z[2] == mimc7.hash2(i["x"], 1)
        assert z[3] == i["chain_id"] and z[4] == mimc7.hash2(i["out_commitment"], asset) and z[5] == i["x"]
        if k == 0:
            ident, empty = [[(w, 1)] for w in range(l + 1)], [[] for _ in range(l + 1)]
            for name, which, extra in (("a", 0, ident), ("b", 1, empty), ("c", 2, empty)):
                assert _rows(getattr(r1, name)) == _oracle_rows(cons, which, extra), name
                assert _rows(getattr(nat, name)) == _rows(getattr(r1, name)), name
    i = ins[2]
    assert circuit.claim_out_leaf(i["out_commitment"], i["amount"], i["token"], ctx) == _spec(i, depth)[3][4]


def case_claim_end_to_end(ctx, depth, n=4, seed=2, key=None):
    """records -> proofs: the C restatement's bytes, the generic prover's bytes from the generated witnesses; og_verify and
    og_verify_batch_d (under og_vk_load, n_pub = 4) accept the four returned inputs; refused with any one input changed and with a
    neighbour's inputs"""
    from oracle.c import binding as oc
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    ins = edge_inputs(rnd, depth, 5)[:n]
    recs = np.stack([_pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    proofs, pub = circuit.claim_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True)
    wit_d = circuit.claim_witness(ctx, depth, ctx.to_device(recs))
    wit = ctx.to_host(wit_d)
    assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:5]).tobytes()
    assert circuit.claim_prove(ctx, pk, depth, ctx.to_device(recs), rs).tobytes() == proofs.tobytes()    # public_out = NULL
    assert pk.prove_batch_device(wit_d, rs).tobytes() == proofs.tobytes()                               # the generic entry point
    ck = oc.prepared_key_from_blob(blob)
    vkb = g16.vk_to_bytes(vk)
    lib = ctx._lib
    for t, i in enumerate(ins):
        assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"claim proof {t} differs from the C restatement"
        good = api.bytes_to_ints(pub[t])
        assert good == _spec(i, depth)[3][1:5]
        p = proofs[t].tobytes()
        assert g16.verify(vkb, good, p, lib=lib) is True
        for slot in range(4):          # root, nullifier_hash, chain_id, out_leaf: each + 1
            forged = list(good)
            forged[slot] = (forged[slot] + 1) % R
            assert g16.verify(vkb, forged, p, lib=lib) is False, slot
    if n > 1:
        assert g16.verify(vkb, pub[1], proofs[0].tobytes(), lib=lib) is False
    with g16.VerifyingKey(ctx, vkb) as dvk:
        assert dvk.n_pub == 4
        assert dvk.verify_batch(pub, proofs).all()
        if n > 1:
            assert not dvk.verify_batch(np.roll(pub, 1, axis=0), proofs).any()       # every proof against a neighbour's inputs
    close()


def forgeries(rnd, depth):
    """(honest request, [(name, z, the rows that must fail)]): four witnesses that are wrong in one place each, every other wire what
    an honest prover's would be (tests/claim_spec.py build(forge=...)).
    the second key: the bits, the wire x and the nullifier hash of x + l for an x < 2^251 - l (asserted), so the recomposition holds,
      P = (x + l) BASE is the note's key and the root is the tree's -- only the comparison fails: first at the highest bit where x + l
      has a 1 and l - 1 a 0, and again at every later 0-bit of l - 1 under a 1-bit of x + l for as long as t stays 1;
    a bit wire equal to 2: bit 0 of an x = 2 (mod 4) becomes 2 and bit 1 gives way, so the recomposition still holds, and every wire
      of the multiplication follows the rows with b = 2 -- only the booleanity row of bit 0 fails;
    an out_leaf that carries another amount: wire 4 = H(out_commitment, H(amount + 1, token)) over honest gadgets -- only the output
      row of the out_leaf gadget fails;
    another token: the out_leaf gadget's values are those of H(out_commitment, H(amount, token + 1)), but its rows name the ONE asset
      wire -- the two rows of the second permutation's first round that read the right input, and the output row, fail"""
    seed_x = rnd.randrange((1 << 251) - ELL)
    assert seed_x < (1 << 251) - ELL
    honest = _inputs(rnd, depth, x=seed_x)
    m, _l, cons, _z = _spec(honest, depth)
    second = seed_x + ELL
    assert second < (1 << 251)
    z = _spec(honest, depth, forge={"bits": [(second >> i) & 1 for i in range(spec.N_BITS)], "x": second})[3]
    top = next(i for i in reversed(range(spec.N_BITS)) if (second >> i) & 1 != (spec.M >> i) & 1)
    assert (second >> top) & 1 == 1, "x + l is above l - 1"
    rows, t = [], 1                 # the comparison, walked here: a 0-bit of l - 1 under a 1-bit of x + l fails while t is still 1
    for i in reversed(range(spec.N_BITS)):
        b = (second >> i) & 1
        if (spec.M >> i) & 1:
            t &= b
        elif b and t:
            rows.append(spec.ROW_CMP + (spec.N_BITS - 1 - i))
    assert rows and rows[0] == spec.ROW_CMP + (spec.N_BITS - 1 - top)
    out = [("the second key x + l", z, rows)]
    even = _inputs(rnd, depth, x=(rnd.randrange(ELL >> 2) << 2) | 2)
    bits = [(even["x"] >> i) & 1 for i in range(spec.N_BITS)]
    bits[0], bits[1] = 2, 0
    z = _spec(even, depth, forge={"bits": bits})[3]
    cons_even = _spec(even, depth)[2]
    out.append(("a bit wire equal to 2", z, [spec.ROW_MUL]))
    larger = mimc7.hash2(honest["out_commitment"], mimc7.hash2(honest["amount"] + 1, honest["token"]))
    g = spec.gadget_row(depth, 4 + depth)
    out.append(("an out_leaf for another amount", _spec(honest, depth, forge={"out_leaf": larger})[3], [g + 729]))
    out.append(("another token", _spec(honest, depth, forge={"out_asset_token": honest["token"] + 1})[3], [g + 365, g + 368, g + 729]))
    for name, z, rows in out:
        c = cons_even if name == "a bit wire equal to 2" else cons
        assert len(z) == m and _failing(c, z) == rows, (name, _failing(c, z), rows)
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


def _tob(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _siblings(depth, leaves, index):
    levels = mimc7.tree_build(leaves + [0] * ((1 << depth) - len(leaves)))
    return [levels[l][(index >> l) ^ 1] for l in range(depth)], levels[-1][0]


def case_the_theft_is_closed(ctx, depth=2, seed=5):
    """an owned note is sealed and its leaf appended.  The sender knows e, pk, S = e pk, t and P; a claim record built from all of it
    -- its best x' is t mod l, the only scalar it holds -- publishes a root that is not the tree's, so the ledger refuses the proof
    whatever it proves.  The payee's record publishes the tree's root.  (The ordinary note of tests/note_spec.py fails this: its
    nullifier' and secret' are functions of S.)"""
    from owshen_amd import api, circuit
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
    # everything the sender knows
    s = bj.multiply(pk, e)
    _tag, t, _pa, _pt = note_spec.kdf(s)
    p = note_spec.one_time_key(pk, t)
    assert mimc7.hash2(*p) == c, "the sender can compute P and c"
    common = dict(amount=amount, index=1, siblings=sib, token=token, chain_id=1, out_commitment=rnd.randrange(R))
    thief = dict(common, x=t % ELL)
    payee = dict(common, x=(sk + t) % ELL)
    assert bj.multiply(bj.BASE, thief["x"]) != p and bj.multiply(bj.BASE, payee["x"]) == p
    wit = ctx.to_host(circuit.claim_witness(ctx, depth, ctx.to_device(np.stack([_pack(circuit, thief), _pack(circuit, payee)]))))
    pub_thief, pub_payee = api.bytes_to_ints(wit[0, 1:5]), api.bytes_to_ints(wit[1, 1:5])
    assert pub_thief[0] != root_py, "the sender's record publishes the tree's root"
    assert pub_payee[0] == root_py and pub_payee[1] == mimc7.hash2(payee["x"], 1)
    assert pub_thief == _spec(thief, depth)[3][1:5] and pub_payee == _spec(payee, depth)[3][1:5]


def case_record_boundary(ctx, depth, seed=4, key=None, other_keys=True):
    """one bad record per case: OG_ERR_INVALID names the record and its lowest offending field, from og_claim_witness_d and from
    og_claim_prove_batch_d; x = l is refused and x = l - 1 taken; the largest well-formed record passes; a transfer key is refused"""
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
            x[rec, FIELDS.index(name) if name in FIELDS else 6 + int(name[1:])] = le(value)
        return x

    bad_cases = [(with_fields(f % nrec, **{name: R}), f % nrec, f, name) for f, name in enumerate(FIELDS)]
    bad_cases += [(with_fields(1, **{f"s{l}": R}), 1, 6 + l, f"sibling {l}") for l in range(depth)]
    bad_cases += [
        (with_fields(2, x=ELL), 2, 0, "x"),
        (with_fields(0, x=ELL + 1), 0, 0, "x"),
        (with_fields(1, x=1 << 251), 1, 0, "x"),
        (with_fields(3, index=1 << depth), 3, 5, "index"),
        (with_fields(1, amount=1 << 128), 1, 1, "amount"),
        (with_fields(2, amount=1 << 128, x=ELL, out_commitment=R), 2, 0, "x"),       # three fields offend: the lowest is named
        (with_fields(3, index=1 << depth, **{f"s{depth - 1}": R}), 3, 5, "index"),
    ]
    for k, (packed, rec, field, name) in enumerate(bad_cases):
        for call in (lambda d: circuit.claim_witness(ctx, depth, d), lambda d: circuit.claim_prove(ctx, pk, depth, d, rs)):
            with pytest.raises(api.OwshenGpuError) as e:
                call(ctx.to_device(packed))
            assert e.value.code == -1 and f"input record {rec}: field {field} ({name})" in str(e.value), (k, str(e.value))
    edge = with_fields(0, x=ELL - 1, amount=TOP, index=(1 << depth) - 1, token=R - 1, chain_id=R - 1, out_commitment=R - 1,
                       **{f"s{depth - 1}": R - 1})
    circuit.claim_witness(ctx, depth, ctx.to_device(edge))
    if other_keys:
        from tests import transfer_cases
        _b, _v, other, close_other = transfer_cases._key(ctx, depth)
        assert other.n_pub == 5
        with pytest.raises(api.OwshenGpuError) as e:
            circuit.claim_prove(ctx, other, depth, ctx.to_device(good), rs)
        assert e.value.code == -1 and "not for this claim-statement shape" in str(e.value), str(e.value)
        close_other()
    close()


def case_second_slab(ctx, depth=2, seed=7):
    """the slab loop past its first slab (tests/statement_slab_cases.py, for this statement): OG_SLAB_MAX = 2 makes three slabs of five
    requests; the profiler counts three witness launches, proofs and public outputs are those of the one-slab call, and a malformed
    record 3 is named by its index in the call.  `ctx` reads the hooks."""
    from owshen_amd import api, circuit
    from tests.statement_slab_cases import _env
    rnd = random.Random(seed)
    blob, vk, pk, close = _key(ctx, depth)
    recs = np.stack([_pack(circuit, i) for i in edge_inputs(rnd, depth, 5)])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(5)]

    def witness_calls(call):
        ctx.profile(True)
        try:
            out = call()
            return out, ctx.profile_read()["witness"][1]
        finally:
            ctx.profile(False)

    (proofs, pub), slabs = witness_calls(lambda: circuit.claim_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True))
    assert slabs == 1
    with _env(OG_SLAB_MAX="2"):
        (p2, pub2), slabs = witness_calls(lambda: circuit.claim_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True))
        assert slabs == 3, f"OG_SLAB_MAX=2 gave {slabs} slabs for 5 requests, not 3"
        assert p2.tobytes() == proofs.tobytes() and pub2.tobytes() == pub.tobytes()
        bad = recs.copy()
        bad[3, 0] = np.frombuffer(ELL.to_bytes(32, "little"), dtype=np.uint8)
        with pytest.raises(api.OwshenGpuError) as e:
            circuit.claim_prove(ctx, pk, depth, ctx.to_device(bad), rs)
        assert e.value.code == -1 and "input record 3: field 0 (x)" in str(e.value), str(e.value)
    close()


def case_through_the_pool(ctx, depth=2, seed=6):
    """seal_owned to a key from og_eddsa_pubkey_batch_d -> og_mimc7_append_d -> scan_owned (a second wallet gets hit 0; the ordinary
    scan answers 0 on the owned memo, scan_owned answers 0 on an ordinary one) -> claim -> og_verify -> the ledger appends out_leaf ->
    `withdraw` of the out note verifies under the new root"""
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed)
    lib = ctx._lib
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))
    sk, sk_other = rnd.randrange(1, R), rnd.randrange(1, R)
    pk_d, _c, ok = ctx.eddsa_pubkey(ctx.to_device(_tob([sk])), compressed=False)
    assert ok.tolist() == [1]
    pk = tuple(toi(pk_d))
    token, chain_id, amount = rnd.randrange(1 << 160), 1387, 9
    req = ctx.to_device(_tob([rnd.randrange(1, R), *pk, amount, token]).reshape(1, 5, 32))
    memos_d, notes_d, ok = ctx.note_seal_owned(req)
    assert ok.tolist() == [1]
    c, leaf = toi(notes_d)
    leaves = [rnd.randrange(R), leaf]
    frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(_tob(leaves)))
    sib, root_py = _siblings(depth, leaves, 1)
    assert toi(root) == [root_py]
    leaf_d = ctx.to_device(_tob([leaf]))
    # the scans
    assert ctx.note_scan_owned(sk_other, memos_d, leaf_d)[1].tolist() == [0]
    assert ctx.note_scan(sk, memos_d, leaf_d)[1].tolist() == [0], "the ordinary scan sees an owned memo"
    plain_memos_d, _n, ok = ctx.note_seal(req)
    assert ok.tolist() == [1] and ctx.note_scan(sk, plain_memos_d, None)[1].tolist() == [1]
    assert ctx.note_scan_owned(sk, plain_memos_d, None)[1].tolist() == [0], "the owned scan sees an ordinary memo"
    opened_d, hit = ctx.note_scan_owned(sk, memos_d, leaf_d)
    assert hit.tolist() == [1]
    x, got_amount, got_token, got_c = toi(opened_d)
    assert (got_amount, got_token, got_c) == (amount, token, c)
    assert note_spec.scan_owned(sk, tuple(toi(memos_d)), leaf) == (1, (x, amount, token, c))
    # the claim: the whole note into an ordinary one only the claimant opens
    out = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R))
    rec = dict(x=x, amount=amount, index=1, siblings=sib, token=token, chain_id=chain_id, out_commitment=mimc7.hash2(out["nullifier"], out["secret"]))
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    _b, vk, pk_c, close = _key(ctx, depth)
    proof, pub = circuit.claim_prove(ctx, pk_c, depth, ctx.to_device(_pack(circuit, rec)[None]), rs, return_public=True)
    c_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), c_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert c_pub[0] == root_py and c_pub[1] == mimc7.hash2(x, 1) and c_pub[2] == chain_id
    assert c_pub[3] == withdraw_spec.leaf_of(out["nullifier"], out["secret"], amount, token)
    # the ledger appends out_leaf; the claimant withdraws the out note
    frontier, root = ctx.mimc7_append(depth, frontier, len(leaves), ctx.to_device(np.ascontiguousarray(pub[0, 3:4])))
    leaves.append(c_pub[3])
    sib_out, root_py = _siblings(depth, leaves, 2)
    assert toi(root) == [root_py]
    from tests.transfer_cases import _key as _other_key
    _b, vk, pk_w, close = _other_key(ctx, depth, "withdraw")
    wrec = circuit.pack_inputs(out["nullifier"], out["secret"], amount, 9, 0, 2, sib_out, token=token, chain_id=chain_id)
    proof, pub = circuit.prove_from_inputs(ctx, pk_w, depth, ctx.to_device(wrec[None]), rs, return_public=True)
    w_pub = api.bytes_to_ints(pub[0])
    assert w_pub[0] == root_py and w_pub[3] == amount
    assert g16.verify(g16.vk_to_bytes(vk), w_pub, proof[0].tobytes(), lib=lib) is True
    close()
