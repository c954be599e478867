"""Join-statement cases shared by the CPU-interpreter run and the GPU run: the product's two R1CS builders and the HIP witness
kernel (two lanes per request) against the plain restatement in tests/join_spec.py, then proofs -- byte-identical to the C
restatement's, accepted by og_verify for the five public inputs and refused for anything else --, three forged witnesses that must
stay unprovable, two notes under different roots, and the boundary check of the records."""
import random

import numpy as np
import pytest

from oracle.py import fields, mimc7
from tests import join_spec as spec
from tests.withdraw_cases import _rows, _oracle_rows

R = fields.R
TOP = (1 << 128) - 1
_TOXIC = (15, 16, 17, 18, 19)
FIELDS = ("nullifier_a", "secret_a", "amount_a", "index_a", "nullifier_b", "secret_b", "amount_b", "index_b", "token", "chain_id",
          "out_commitment")


def paired_paths(rnd, depth, k, low_a=None, low_b=None, high=None):
    """Two paths that meet: random independent paths do not share a root.  Below level k each note gets its own random siblings
    (and index bits low_a / low_b, random if None); AT level k each note's sibling is the other's node, with index bits 0 (a) and
    1 (b); above level k siblings and index bits (`high`, random if None) are shared.  The nodes at level k depend on the leaves, so
    this returns bind(leaf_a, leaf_b) -> dict(index_a, siblings_a, index_b, siblings_b); the spec's own assertion shows that the
    two roots agree."""
    assert 0 <= k < depth
    low = [rnd.randrange(1 << k) if v is None else v for v in (low_a, low_b)]
    high = rnd.randrange(1 << (depth - 1 - k)) if high is None else high
    assert all(0 <= v < (1 << k) for v in low) and 0 <= high < (1 << (depth - 1 - k))
    below = [[rnd.randrange(R) for _ in range(k)] for _ in range(2)]
    above = [rnd.randrange(R) for _ in range(depth - 1 - k)]
    index = [low[x] | (x << k) | (high << (k + 1)) for x in range(2)]

    def bind(leaf_a, leaf_b):
        node = [mimc7.merkle_root_from_path(leaf, low[x], below[x])[-1] for x, leaf in enumerate((leaf_a, leaf_b))]
        return dict(index_a=index[0], siblings_a=below[0] + [node[1]] + above, index_b=index[1], siblings_b=below[1] + [node[0]] + above)

    return bind


def _leaf(i, x):
    return mimc7.hash2(mimc7.hash2(i["nullifier_" + x], i["secret_" + x]), mimc7.hash2(i["amount_" + x], i["token"]))


def _inputs(rnd, depth, k=None, low_a=None, low_b=None, high=None, **values):
    """one well-formed request (the keyword arguments of spec.build / circuit.pack_join_inputs): random notes with amounts below
    2^64, `values` over them, and paths that diverge at level k (random if None)"""
    i = dict(nullifier_a=rnd.randrange(R), secret_a=rnd.randrange(R), amount_a=rnd.randrange(1, 1 << 64), nullifier_b=rnd.randrange(R),
             secret_b=rnd.randrange(R), amount_b=rnd.randrange(1, 1 << 64), token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32),
             out_commitment=rnd.randrange(R))
    i.update(values)
    bind = paired_paths(rnd, depth, rnd.randrange(depth) if k is None else k, low_a, low_b, high)
    i.update(bind(_leaf(i, "a"), _leaf(i, "b")))
    return i


def edge_inputs(rnd, depth, n):
    """n >= 5 requests; the first five carry, by construction: divergence at level 0 with indices 0 and 1; divergence at the top
    level with index_b the last leaf; amount_a = 2^128 - 1 with amount_b = 0 (the largest joined note); amount_a = 0 = amount_b;
    nullifier_a = secret_a = out_commitment = r - 1"""
    assert n >= 5
    return [_inputs(rnd, depth, k=0, high=0),
            _inputs(rnd, depth, k=depth - 1, low_b=(1 << (depth - 1)) - 1),
            _inputs(rnd, depth, amount_a=TOP, amount_b=0),
            _inputs(rnd, depth, amount_a=0, amount_b=0),
            _inputs(rnd, depth, nullifier_a=R - 1, secret_a=R - 1, out_commitment=R - 1)] + [_inputs(rnd, depth) for _ in range(n - 5)]


def _pack(circuit, i):
    return circuit.pack_join_inputs(**i)


def _spec(i, depth, forge=None):
    return spec.build(depth, forge=forge, **i)


def _wit_bytes(z):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(1, -1, 32).copy()


def _key(ctx, depth, statement="join"):
    """(key blob, vk, loaded key, close) of the join statement (or the split statement) at `depth`.  On the CPU interpreter set-up
    and the key upload take tens of seconds, so there the cases of a session share one key per shape and `close` does nothing
    (as tests/split_cases._key); on the GPU every case loads and frees its own."""
    from owshen_amd import circuit, groth16 as g16
    shared = type(ctx).__module__ == "tests.emu"
    cache = ctx.__dict__.setdefault("_join_keys", {}) if shared else {}
    k = (statement, depth)
    if k not in cache:
        r1 = circuit.join_r1cs(ctx.mimc7_constants(), depth) if statement == "join" else circuit.split_r1cs(ctx.mimc7_constants(), depth)
        blob, vk = g16.setup(ctx, r1, *_TOXIC)
        cache[k] = (blob, vk, g16.ProvingKey(ctx, blob))
    blob, vk, pk = cache[k]
    return blob, vk, pk, (lambda: None) if shared else pk.close


def case_r1cs_and_witness_match_spec(ctx, depth, n, seed=1):
    """both builders give the spec's rows, og_join_shape is the spec's shape, and the kernel's witness is the spec's z integer for
    integer -- over the edge requests of `edge_inputs`"""
    import ctypes as C
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    ins = edge_inputs(rnd, depth, n)
    assert (ins[0]["index_a"], ins[0]["index_b"]) == (0, 1) and ins[1]["index_b"] == (1 << depth) - 1
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_join_shape(depth, shp))
    assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.join_shape(depth) and int(shp[2]) == spec.N_PUB == 5
    r1 = circuit.join_r1cs(ctx.mimc7_constants(), depth)
    nat = circuit.join_r1cs_native(ctx, depth)
    assert (nat.n_wires, nat.n_pub, nat.n_constraints, nat.log_d) == (r1.n_wires, r1.n_pub, r1.n_constraints, r1.log_d)
    assert (r1.n_wires, r1.n_constraints) == spec.shape(depth) and r1.n_pub == 5
    wit = ctx.to_host(circuit.join_witness(ctx, depth, ctx.to_device(np.stack([_pack(circuit, i) for i in ins]))))
    for k, i in enumerate(ins):
        m, l, cons, z = _spec(i, depth)
        assert (m, l) == (r1.n_wires, r1.n_pub) and len(cons) == r1.n_constraints
        got = api.bytes_to_ints(wit[k])
        assert got == z, f"join witness {k}: first differing wire {next(w for w in range(m) if got[w] != z[w])}"
        total = i["amount_a"] + i["amount_b"]
        assert z[1] == mimc7.merkle_root_from_path(_leaf(i, "a"), i["index_a"], i["siblings_a"])[-1]
        assert z[1] == mimc7.merkle_root_from_path(_leaf(i, "b"), i["index_b"], i["siblings_b"])[-1]
        assert z[2:5] == [mimc7.hash2(i["nullifier_a"], 0), mimc7.hash2(i["nullifier_b"], 0), i["chain_id"]] and z[14] == total
        assert z[5] == mimc7.hash2(i["out_commitment"], mimc7.hash2(total, i["token"])), "out_leaf"
        assert (z[2] - z[3]) * z[15] % R == 1
        if k == 0:
            ident, empty = [[(w, 1)] for w in range(l + 1)], [[] for _ in range(l + 1)]
            for name, which, extra in (("a", 0, ident), ("b", 1, empty), ("c", 2, empty)):
                assert _rows(getattr(r1, name)) == _oracle_rows(cons, which, extra), name
                assert _rows(getattr(nat, name)) == _rows(getattr(r1, name)), name
    # the ledger's and the receiver's side: the joined leaf through og_mimc7_hash2_d
    i = ins[4]
    assert circuit.join_out_leaf(i["out_commitment"], i["amount_a"] + i["amount_b"], i["token"], ctx) == _spec(i, depth)[3][5]


def case_join_end_to_end(ctx, depth, n=4, seed=2, key=None):
    """records -> proofs: the C restatement's bytes, the generic prover's bytes from the generated witnesses, og_verify accepts the
    five returned inputs and refuses root + 1, either nullifier hash + 1, out_leaf + 1, and proof 0 against request 1's inputs"""
    from oracle.c import binding as oc
    from owshen_amd import api, circuit, groth16 as g16
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    ins = edge_inputs(rnd, depth, 5)[:n]
    recs = np.stack([_pack(circuit, i) for i in ins])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in ins]
    proofs, pub = circuit.join_prove(ctx, pk, depth, ctx.to_device(recs), rs, return_public=True)
    wit_d = circuit.join_witness(ctx, depth, ctx.to_device(recs))
    wit = ctx.to_host(wit_d)
    assert pub.tobytes() == np.ascontiguousarray(wit[:, 1:6]).tobytes()
    assert circuit.join_prove(ctx, pk, depth, ctx.to_device(recs), rs).tobytes() == proofs.tobytes()        # public_out = NULL
    assert pk.prove_batch_device(wit_d, rs).tobytes() == proofs.tobytes()                                  # the generic entry point
    ck = oc.prepared_key_from_blob(blob)
    vkb = g16.vk_to_bytes(vk)
    lib = ctx._lib
    for t, i in enumerate(ins):
        assert proofs[t].tobytes() == ck.prove(wit[t], *rs[t]), f"join proof {t} differs from the C restatement"
        z = _spec(i, depth)[3]
        good = api.bytes_to_ints(pub[t])
        assert good == z[1:6]
        p = proofs[t].tobytes()
        assert g16.verify(vkb, good, p, lib=lib) is True
        for slot in (0, 1, 2, 4):          # root + 1, nullifier_hash_a + 1, nullifier_hash_b + 1, out_leaf + 1
            forged = list(good)
            forged[slot] = (forged[slot] + 1) % R
            assert g16.verify(vkb, forged, p, lib=lib) is False, slot
    assert g16.verify(vkb, pub[1], proofs[0].tobytes(), lib=lib) is False
    close()


def _failing(cons, z):
    def val(lc):
        return sum(c * z[w] for w, c in lc.items()) % R

    return [k for k, (a, b, c) in enumerate(cons) if val(a) * val(b) % R != val(c)]


def forgeries(rnd, depth):
    """(honest request, [(name, z, the one row that must fail)]): three witnesses that are wrong in exactly one row each, every
    other wire what an honest prover's would be (tests/join_spec.py build(forge=...)).
    inflated sum: sum = amount_a + amount_b + 1 with its bits and both output gadgets following -- only the sum row (1) fails;
    wrapped input: amount_b = r - 1 = -1, so sum = amount_a - 1 holds in the field; note b's asset, leaf and path follow, and note
      a's siblings come from paired_paths over the forged leaf so that both walks still reach one root; the bit wires are the low
      128 bits -- only the recomposition of amount_b (260) fails;
    the same note twice: note b is a copy of note a (one path, one nullifier hash) with nh_diff_inv = 0 -- only the
      distinctness row (2) fails"""
    honest = _inputs(rnd, depth)
    out = []
    m, _l, cons, z = _spec(honest, depth, forge={"sum": honest["amount_a"] + honest["amount_b"] + 1})
    out.append(("inflated sum", z, 1))
    wrapped = _inputs(rnd, depth, amount_b=R - 1)
    _m, _l, _c, z = _spec(wrapped, depth, forge={})
    assert z[11] == R - 1 and z[14] == wrapped["amount_a"] - 1
    out.append(("wrapped input", z, 260))
    twice = dict(honest, nullifier_b=honest["nullifier_a"], secret_b=honest["secret_a"], amount_b=honest["amount_a"],
                 index_b=honest["index_a"], siblings_b=honest["siblings_a"])
    _m, _l, _c, z = _spec(twice, depth, forge={"nh_diff_inv": 0})
    assert z[2] == z[3] and z[14] == 2 * honest["amount_a"]
    out.append(("the same note twice", z, 2))
    for name, z, row in out:
        assert len(z) == m and _failing(cons, z) == [row], (name, _failing(cons, z))
    return honest, out


def case_forgeries_are_unprovable(ctx, depth, seed=3, key=None):
    """each forged witness fails exactly its row on the CPU, and og_prove_batch_d answers OG_ERR_UNSATISFIED for it; the honest
    witness proves"""
    from owshen_amd import api
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    honest, forged = forgeries(rnd, depth)
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    for name, z, _row in forged:
        with pytest.raises(api.OwshenGpuError) as e:
            pk.prove_batch_device(ctx.to_device(_wit_bytes(z)), rs)
        assert e.value.code == -4, (name, str(e.value))
    assert pk.prove_batch_device(ctx.to_device(_wit_bytes(_spec(honest, depth)[3])), rs).shape == (1, 256)
    close()


def case_different_roots(ctx, depth, seed=5, key=None):
    """a well-formed record whose note b has a foreign sibling: nothing at the boundary can see it -- og_join_witness_d succeeds with
    wire 1 = note a's root -- and og_join_prove_batch_d answers OG_ERR_UNSATISFIED through the prover's row check"""
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    blob, vk, pk, close = key if key is not None else _key(ctx, depth)
    i = _inputs(rnd, depth)
    foreign = dict(i, siblings_b=i["siblings_b"][:-1] + [rnd.randrange(R)])
    root_a = mimc7.merkle_root_from_path(_leaf(i, "a"), i["index_a"], i["siblings_a"])[-1]
    assert mimc7.merkle_root_from_path(_leaf(i, "b"), foreign["index_b"], foreign["siblings_b"])[-1] != root_a
    rec = _pack(circuit, foreign)[None]
    wit = ctx.to_host(circuit.join_witness(ctx, depth, ctx.to_device(rec)))
    assert api.bytes_to_ints(wit[0][1:2]) == [root_a]
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    with pytest.raises(api.OwshenGpuError) as e:
        circuit.join_prove(ctx, pk, depth, ctx.to_device(rec), rs)
    assert e.value.code == -4, str(e.value)
    assert circuit.join_prove(ctx, pk, depth, ctx.to_device(_pack(circuit, i)[None]), rs).shape == (1, 256)
    close()


def case_record_boundary(ctx, depth, seed=4, key=None, other_keys=True):
    """one bad field per case: OG_ERR_INVALID names the record and its lowest offending field, from og_join_witness_d and from
    og_join_prove_batch_d; the largest well-formed record passes; keys of another shape are refused"""
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
        """sa<l> / sb<l>: sibling l of note a / b"""
        x = good.copy()
        for name, value in fv.items():
            field = FIELDS.index(name) if name in FIELDS else 11 + (depth if name[1] == "b" else 0) + int(name[2:])
            x[rec, field] = le(value)
        return x

    bad_cases = [
        (with_fields(3, secret_b=R), 3, 5, "secret_b"),
        (with_fields(1, amount_a=1 << 128), 1, 2, "amount_a"),
        (with_fields(2, amount_a=TOP - 6, amount_b=7), 2, 6, "amount_b"),                   # amount_a + amount_b = 2^128
        (with_fields(3, index_b=1 << depth), 3, 7, "index_b"),
        (with_fields(2, **{f"sb{depth - 1}": R}), 2, 11 + 2 * depth - 1, f"sibling b {depth - 1}"),
        (with_fields(0, nullifier_b=ins[0]["nullifier_a"]), 0, 4, "nullifier_b"),
        (with_fields(1, amount_b=1 << 128, index_a=1 << depth, out_commitment=R), 1, 3, "index_a"),   # three fields offend: the lowest is named
    ]
    for k, (packed, rec, field, name) in enumerate(bad_cases):
        for call in (lambda d: circuit.join_witness(ctx, depth, d), lambda d: circuit.join_prove(ctx, pk, depth, d, rs)):
            with pytest.raises(api.OwshenGpuError) as e:
                call(ctx.to_device(packed))
            assert e.value.code == -1 and f"input record {rec}: field {field} ({name})" in str(e.value), str(e.value)
    # the largest well-formed record passes the boundary
    last = (1 << depth) - 1
    edge = with_fields(0, nullifier_a=R - 1, secret_a=R - 1, amount_a=TOP, index_a=last, nullifier_b=R - 2, secret_b=R - 1, amount_b=0,
                       index_b=last, token=R - 1, chain_id=R - 1, out_commitment=R - 1, **{f"sa{depth - 1}": R - 1, f"sb{depth - 1}": R - 1})
    circuit.join_witness(ctx, depth, ctx.to_device(edge))
    if other_keys:
        for statement, d in (("split", depth), ("join", depth + 1 if depth == 1 else depth - 1)):
            _b, _v, other, close_other = _key(ctx, d, statement)
            with pytest.raises(api.OwshenGpuError) as e:
                circuit.join_prove(ctx, other, depth, ctx.to_device(good), rs)
            assert e.value.code == -1 and "not for this join-statement shape" in str(e.value), str(e.value)
            close_other()
    close()
