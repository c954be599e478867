"""The A and B queries over the QAP rows (include/owshen_gpu.h: og_setup_rows / og_pk_load_rows / og_pk_query_form); cases shared
by the CPU-interpreter run (test_emu_row_form.py) and the GPU run (test_gpu_row_form.py).

sum_i z_i [a_i(tau)] = sum_j (A z)_j [L_j(tau)]: the same group element, so a key loaded with its row-basis extension must give
the bytes the plain blob gives, which the C restatement re-proves from the plain blob.

Circuits of our own, all with 24 constraints (27 QAP rows with the 3 consistency rows, domain 32).  Constraint k is
(sum of fan_a fresh wires) x (sum of fan_b fresh wires) = a fresh wire:
  W   fan 8 | 8   193 A wires against 27 rows, 192 B wires against 24: the rule takes the rows for both queries
  WA  fan 8 | 1   A as in W; 24 B wires against 24 rows: B stays on the wires
  WB  fan 1 | 8   27 A wires against 27 rows: A stays; B over its 24 rows -- the row map is B's own and has no consistency row
The tolerance is none: every comparison is of proof bytes."""
import random

import numpy as np
import pytest

from oracle.py import fields

R = fields.R
N_CONS, N_PUB = 24, 2
TOXIC = (0x1234567, 0x2345678, 0x3456789, 0x456789a, 0x56789ab)
_CACHE = {}


def _wit(z):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(-1, 32).copy()


class Circuit:
    def __init__(self, fan_a, fan_b):
        self.rows, nxt = [], 1
        for _ in range(N_CONS):
            a = list(range(nxt, nxt + fan_a))
            b = list(range(nxt + fan_a, nxt + fan_a + fan_b))
            c = nxt + fan_a + fan_b
            nxt = c + 1
            self.rows.append((a, b, c))
        self.n_wires = nxt

    def r1cs(self):
        from owshen_amd import groth16 as g16
        cons = [({w: 1 for w in a}, {w: 1 for w in b}, {c: 1}) for a, b, c in self.rows]
        return g16.R1CS.from_constraints(self.n_wires, N_PUB, cons)

    def witness(self, seed, a_sum=None, b_sum=None):
        """random wires; a_sum / b_sum(k), if given, is what constraint k's A / B row must add up to"""
        rnd = random.Random(seed)
        z = [1] + [0] * (self.n_wires - 1)
        for k, (a, b, c) in enumerate(self.rows):
            for ws, want in ((a, a_sum), (b, b_sum)):
                for w in ws:
                    z[w] = rnd.randrange(R)
                if want is not None:
                    z[ws[-1]] = (want(k) - sum(z[w] for w in ws[:-1])) % R
            z[c] = sum(z[w] for w in a) * sum(z[w] for w in b) % R
        return _wit(z)


class Key:
    def __init__(self, ctx, fan_a, fan_b):
        from owshen_amd import groth16 as g16
        from tests.r1cs_util import oracle_c_key_from_blob
        self.circuit = Circuit(fan_a, fan_b)
        self.blob, vk = g16.setup(ctx, self.circuit.r1cs(), *TOXIC)
        self.vk = g16.vk_to_bytes(vk)
        assert isinstance(self.blob, bytes) and self.blob.rows is not None and self.blob[:8] == b"OWPK0001"
        assert type(self.blob[8:]) is bytes and type(bytes(self.blob)) is bytes          # a slice / a copy is a plain blob
        self.row = g16.ProvingKey(ctx, self.blob)
        self.plain = g16.ProvingKey(ctx, bytes(self.blob))
        self.oracle = oracle_c_key_from_blob(bytes(self.blob))


def key(ctx, name):
    if (id(ctx), name) not in _CACHE:
        _CACHE[(id(ctx), name)] = (ctx, Key(ctx, *{"W": (8, 8), "WA": (8, 1), "WB": (1, 8)}[name]))
    return _CACHE[(id(ctx), name)][1]


def _rs(n, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(R), rnd.randrange(R)) for _ in range(n)]


def _forms(pk):
    return {q: f["form"] for q, f in pk.query_forms().items()}


def _same_everywhere(ctx, k, zs, rs):
    """row form == plain blob == the C restatement, proof by proof; returns the bytes"""
    got = k.row.prove_batch(zs, rs)
    assert got.tobytes() == k.plain.prove_batch(zs, rs).tobytes()
    for w, (r, s), p in zip(zs, rs, got):
        assert p.tobytes() == k.oracle.prove(w, r, s)
    return got


# ---- 1: the same proofs -------------------------------------------------------------------------------------------------------------
def case_same_proofs(ctx, n):
    k = key(ctx, "W")
    assert _forms(k.row) == {"a": "row", "b1": "row", "b2": "row", "l": "wire", "h": "wire"}
    zs = np.stack([k.circuit.witness(100 + t) for t in range(n)])
    rs = _rs(n, n)
    got = _same_everywhere(ctx, k, zs, rs)
    ctx.set_lanes(1)
    try:
        assert k.row.plan(n)[0] == "serial"
        assert k.row.prove_batch(zs, rs).tobytes() == got.tobytes()
    finally:
        ctx.set_lanes(2)


def case_same_proofs_pipelined(ctx, monkeypatch):
    """9 proofs in sub-batches of 1, 2, 2, 2, 2 through the stage pipeline (hooks build: OG_PIPE_MIN): both scratch slots reused,
    the sorts of A z and B z on the prep stream while the math stream's quotient destroys its own copy of them"""
    k = key(ctx, "W")
    n = 9
    zs = np.stack([k.circuit.witness(200 + t) for t in range(n)])
    rs = _rs(n, 9)
    want = _same_everywhere(ctx, k, zs, rs)
    monkeypatch.setenv("OG_SUB_BATCH", "2")
    monkeypatch.setenv("OG_PIPE_MIN", "1")
    assert k.row.plan(n) == ("stage pipeline", [1, 2, 2, 2, 2])
    assert k.row.prove_batch(zs, rs).tobytes() == want.tobytes()
    assert k.row.prove_batch_device(ctx.to_device(zs), rs).tobytes() == want.tobytes()
    monkeypatch.delenv("OG_PIPE_MIN")
    assert k.row.plan(n) == ("symmetric lanes", [2, 2, 2, 2, 1])
    assert k.row.prove_batch(zs, rs).tobytes() == want.tobytes()


def case_host_chains(ctx):
    k = key(ctx, "W")
    zs = np.stack([k.circuit.witness(300 + t) for t in range(3)])
    rs = _rs(3, 33)
    want = k.plain.prove_batch(zs, rs)
    ctx.set_host_chains(8)
    try:
        assert k.row.prove_batch_device(ctx.to_device(zs), rs).tobytes() == want.tobytes()
    finally:
        ctx.set_host_chains(0)


# ---- 2: the rule ----------------------------------------------------------------------------------------------------------------------
def case_rule_wide_keys(ctx):
    w, wa, wb = key(ctx, "W"), key(ctx, "WA"), key(ctx, "WB")
    fw = w.row.query_forms()
    assert (fw["a"]["points"], fw["b1"]["points"], fw["b2"]["points"]) == (27, 27, 27)    # ONE row list: the rows with an A or a B entry
    assert fw["a"]["table"] == fw["b1"]["table"] == "a" and fw["b2"]["table"] == "b2"      # A and B1 share the G1 Lagrange tables
    assert _forms(wa.row) == {"a": "row", "b1": "wire", "b2": "wire", "l": "wire", "h": "wire"}
    assert wa.row.query_forms()["a"]["points"] == 27 and wa.row.query_forms()["b1"]["points"] == 24
    assert _forms(wb.row) == {"a": "wire", "b1": "row", "b2": "row", "l": "wire", "h": "wire"}
    for k in (w, wa, wb):
        assert _forms(k.plain) == dict.fromkeys(("a", "b1", "b2", "l", "h"), "wire")
        assert k.row.density() == k.plain.density() and k.row.windows() == k.plain.windows()
        assert (k.row.n_wires, k.row.n_pub, k.row.log_d, k.row.n_rows) == (k.circuit.n_wires, N_PUB, 5, 27)
    # (A: the 192 summed wires -- the two public ones among them -- and wire 0 of the consistency rows)
    assert w.row.density() == {"a": 193, "b": 192, "l": w.circuit.n_wires - 3, "h": 31}
    assert w.row.hbm_bytes() < w.plain.hbm_bytes()                      # no wire-form tables for A, B1, B2
    for k in (wa, wb):
        zs = np.stack([k.circuit.witness(400 + t) for t in range(2)])
        _same_everywhere(ctx, k, zs, _rs(2, 44))


def case_rule_natural_withdraw(ctx):
    """the natural depth-2 withdraw statement: no extension is made for it, all five queries stay on the wires, the proofs are
    the C restatement's"""
    from owshen_amd import circuit, groth16 as g16
    from tests.r1cs_util import oracle_c_key_from_blob
    depth = 2
    r1 = circuit.withdraw_r1cs(ctx.mimc7_constants(), depth, 0, 0)
    blob, _vk = g16.setup(ctx, r1, 101, 202, 303, 404, 505)
    assert blob.rows is None
    pk = g16.ProvingKey(ctx, blob)
    assert _forms(pk) == dict.fromkeys(("a", "b1", "b2", "l", "h"), "wire")
    d, f = pk.density(), pk.query_forms()
    # (a table holds the query's own bases, or the few more of a wire list it shares with another query: og_pk_density)
    assert all(d[q[0]] <= f[q]["points"] <= d[q[0]] + 64 for q in ("a", "b1", "b2", "l")) and f["h"]["points"] == d["h"] == (1 << pk.log_d) - 1
    rnd = random.Random(2)
    ins = [dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=7, recipient=9, pad_seed=rnd.randrange(R), index=rnd.randrange(4),
                siblings=[rnd.randrange(R) for _ in range(depth)], token=rnd.randrange(1 << 160), chain_id=1387) for _ in range(2)]
    wit_d = circuit.witness(ctx, depth, ctx.to_device(np.stack([circuit.pack_inputs(**i) for i in ins])), 0, 0)
    wit, rs = ctx.to_host(wit_d), _rs(2, 22)
    ck = oracle_c_key_from_blob(bytes(blob))
    assert [p.tobytes() for p in pk.prove_batch_device(wit_d, rs)] == [ck.prove(np.asarray(wit[t]), *rs[t]) for t in range(2)]
    pk.close()


def case_rule_decides_at_load(ctx, monkeypatch):
    """A key the rule keeps on the wires (the 60-constraint random circuit of tests/groth16_cases.py: 0 / 1 wires, coefficients 1, 2,
    r - 1) handed an extension all the same -- made under OG_ROW_FORM=1, hooks build: the load decides by itself and keeps the
    wires; forced onto the rows too, it proves the same bytes."""
    from owshen_amd import groth16 as g16
    from tests import groth16_cases as gc
    from tests.r1cs_util import oracle_c_key_from_blob
    blob, zs, rs = gc.medium_case(ctx, 60, 3)
    assert blob.rows is None
    monkeypatch.setenv("OG_ROW_FORM", "1")
    forced, _zs, _rs2 = gc.medium_case(ctx, 60, 3)
    assert forced.rows is not None and bytes(forced) == bytes(blob)
    monkeypatch.delenv("OG_ROW_FORM")
    plain, by_rule = g16.ProvingKey(ctx, blob), g16.ProvingKey(ctx, forced)
    assert by_rule.query_forms() == plain.query_forms() and _forms(plain) == dict.fromkeys(("a", "b1", "b2", "l", "h"), "wire")
    monkeypatch.setenv("OG_ROW_FORM", "1")
    on_rows = g16.ProvingKey(ctx, forced)
    monkeypatch.setenv("OG_ROW_FORM", "0")
    off = g16.ProvingKey(ctx, forced)
    monkeypatch.delenv("OG_ROW_FORM")
    assert _forms(on_rows) == {"a": "row", "b1": "row", "b2": "row", "l": "wire", "h": "wire"} and off.query_forms() == plain.query_forms()
    ck = oracle_c_key_from_blob(bytes(blob))
    want = [ck.prove(w, r, s) for w, (r, s) in zip(zs, rs)]
    for pk in (plain, by_rule, on_rows, off):
        assert pk.density() == plain.density() and pk.windows() == plain.windows()
        assert [p.tobytes() for p in pk.prove_batch(zs, rs)] == want
    for pk in (plain, by_rule, on_rows, off):
        pk.close()


# ---- 3: edge scalars --------------------------------------------------------------------------------------------------------------------
def case_edge_scalars(ctx):
    w, wb = key(ctx, "W"), key(ctx, "WB")
    zs = np.stack([
        w.circuit.witness(500, b_sum=lambda k: 0),                                       # every (B z)_j = 0: the query's sum is infinity
        w.circuit.witness(501, a_sum=lambda k: (1, R - 1)[k & 1], b_sum=lambda k: (R - 1, 1)[k & 1]),   # 1 and r - 1: the top-window carry
        w.circuit.witness(502, a_sum=lambda k: 0, b_sum=lambda k: 0),                    # A z = 0 on every constraint row: only the consistency rows count
    ])
    _same_everywhere(ctx, w, zs, _rs(3, 55))
    # a row with no B entry is not in B's map: WB's row list is B's own -- the 24 constraint rows, none of the 3 consistency rows
    f = wb.row.query_forms()
    assert f["b1"]["points"] == f["b2"]["points"] == 24 and wb.row.n_rows == 27
    zs = np.stack([wb.circuit.witness(503), wb.circuit.witness(504, b_sum=lambda k: 0)])
    _same_everywhere(ctx, wb, zs, _rs(2, 56))


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------
def _flip(ext, offset):
    return ext[:offset] + bytes([ext[offset] ^ 1]) + ext[offset + 1:]


def bad_extensions(ctx):
    """name -> (extension, words one of which the refusal must hold)"""
    w, wa = key(ctx, "W"), key(ctx, "WA")
    ext = w.blob.rows
    assert len(ext) == 64 + 27 * 192 and ext[:8] == b"OWPR0001"
    return {
        "truncated by one byte": (ext[:-1], ("length",)),
        "another key's extension": (wa.blob.rows, ("digest",)),
        "one flipped bit in a G1 point": (_flip(ext, 64 + 5 * 64 + 3), ("G1 point", "A query", "B (G1) query")),
        "one flipped bit in a G2 point": (_flip(ext, 64 + 27 * 64 + 7 * 128 + 70), ("G2 point", "B (G2) query")),
    }


BAD = ("truncated by one byte", "another key's extension", "one flipped bit in a G1 point", "one flipped bit in a G2 point")


def case_refusal(ctx, name):
    from owshen_amd import groth16 as g16
    from owshen_amd.api import OwshenGpuError
    w = key(ctx, "W")
    ext, words = bad_extensions(ctx)[name]
    blob = g16.ProvingKeyBlob(w.blob)
    blob.rows = ext
    with pytest.raises(OwshenGpuError) as e:
        g16.ProvingKey(ctx, blob)
    assert e.value.code == -1 and "og_pk_load_rows" in str(e.value) and "row-basis extension" in str(e.value)
    assert any(word in str(e.value) for word in words), str(e.value)
    # the context is usable: the good extension loads and proves
    good = g16.ProvingKey(ctx, w.blob)
    z, rs = w.circuit.witness(600), _rs(1, 66)
    assert good.prove_batch(z[None], rs)[0].tobytes() == w.oracle.prove(z, *rs[0])
    good.close()


# ---- 5: the window-sharded front --------------------------------------------------------------------------------------------------------
def case_sharded(ctx, world, n):
    """every rank's front half played in turn on this device, the blocks laid out as the all-gather leaves them"""
    k = key(ctx, "W")
    zs = np.stack([k.circuit.witness(700 + 10 * world + t) for t in range(n)])
    rs = _rs(n, 77 + world)
    zs_d = ctx.to_device(zs)
    want = k.plain.prove_batch_device(zs_d, rs)
    parts = [np.array(ctx.to_host(k.row.prove_partials_device(zs_d, r, world)).reshape(-1), copy=True) for r in range(world)]
    got = k.row.prove_from_partials(ctx.to_device(np.concatenate(parts)), world, rs)
    assert got.tobytes() == want.tobytes()
    assert got[0].tobytes() == k.oracle.prove(zs[0], *rs[0])
