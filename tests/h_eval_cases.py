"""The quotient in the evaluation form (include/owshen_gpu.h: OG_QUERY_FORM_EVAL); cases shared by the
CPU-interpreter run (test_emu_h_eval.py) and the GPU run (test_gpu_h_eval.py).

A key in this form keeps h on the coset: its H tables hold the DFT of the H query, its L tables carry C z.  The group element
sum_k h_k H_k is the same, so the proof bytes are.  Every comparison here is of proof bytes and the tolerance is none.  Each
circuit compares three things, proof by proof: the key in the evaluation form (hooks build: OG_H_FORM=1), the SAME blob loaded
with OG_H_FORM=0, and the C restatement proving from the plain blob.  The reference -- nine witnesses, nine (r, s), the C
restatement's nine proofs -- is made once per circuit and shared by every schedule.

The witnesses are random, so (a b)(x) and c(x) each have a non-zero x^(d-1) coefficient -- the coefficient that has no H point and
is dropped from both the H tables and the fold of C: every case exercises the cancellation of the two, which holds because the
witness satisfies the circuit (h has degree <= d - 2).

Circuits:
  W    tests/row_form_cases.py's, domain 32: one stage block.  Loaded WITH its row-basis extension (og_pk_load_rows): A and B
       over the rows, L and H in the evaluation form
  D11  1100 constraints w x w' = w'', domain 2^11: two stage blocks, the second a single stage
  WD   the depth-2 withdraw statement
  PC   24 constraints of our own for the public and constant terms of the fold (PcCircuit)
KEYS of D11 and WD are loaded on the GPU only: the load-time DFT over points is d log d scalar multiplications of 254 bits,
25 s and 108 s on the interpreter at these domains.  Their stage-block shapes run on the interpreter too, through the quotient's
half of the form alone (case_coset_pipeline_shapes: 2^11, 2^12, 2^13 against og_ntt_fr_d and a product of integers).
"""
import contextlib
import os
import random

import numpy as np
import pytest

from oracle.py import fields
from tests import row_form_cases as rc

R = fields.R
N = 9   # witnesses per circuit: what the stage-pipeline case needs; the other schedules prove a prefix
_CACHE = {}


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class PcCircuit:
    """24 constraints, 2 public wires, every product's factors fresh wires:
      k = 0, 1   x x' = PUBLIC wire 1 | 2                        (C entries on public wires: bases the L query never had)
      k = 2      x x' = 5 . wire 0                               (a C entry on the constant wire)
      k = 3      x x' = (r-1) u + (r-1) u' + (r-1) u'' + o       (one C row with several entries of coefficient r - 1)
      k >= 4     x x' = o
    """
    N_CONS, N_PUB = 24, 2

    def __init__(self):
        self.cons, nxt = [], 3
        for k in range(self.N_CONS):
            a, b = nxt, nxt + 1
            nxt += 2
            if k < 2:
                c = {k + 1: 1}
            elif k == 2:
                c = {0: 5}
            elif k == 3:
                c = {nxt: R - 1, nxt + 1: R - 1, nxt + 2: R - 1, nxt + 3: 1}
                nxt += 4
            else:
                c = {nxt: 1}
                nxt += 1
            self.cons.append(({a: 1}, {b: 1}, c))
        self.n_wires = nxt

    def r1cs(self):
        from owshen_amd import groth16 as g16
        return g16.R1CS.from_constraints(self.n_wires, self.N_PUB, self.cons)

    def witness(self, seed):
        rnd = random.Random(seed)
        z = [1] + [0] * (self.n_wires - 1)
        for k, (a, b, c) in enumerate(self.cons):
            (wa,), (wb,) = a, b
            z[wa] = rnd.randrange(1, R)
            z[wb] = 5 * pow(z[wa], -1, R) % R if k == 2 else rnd.randrange(R)
            p = z[wa] * z[wb] % R
            if k == 2:
                assert p == 5
            elif k == 3:
                ws = sorted(c)
                for w in ws[:3]:
                    z[w] = rnd.randrange(R)
                z[ws[3]] = (p + sum(z[w] for w in ws[:3])) % R
            else:
                (w,) = c
                z[w] = p
        for a, b, c in self.cons:
            dot = lambda lc: sum(v * z[w] for w, v in lc.items()) % R
            assert dot(a) * dot(b) % R == dot(c)
        return rc._wit(z)


def _build_w(ctx):
    k = rc.key(ctx, "W")
    return k.blob, np.stack([k.circuit.witness(900 + t) for t in range(N)])


def _build_d11(ctx):
    from owshen_amd import groth16 as g16
    n = 1100
    cons = [({1 + 3 * k: 1}, {2 + 3 * k: 1}, {3 + 3 * k: 1}) for k in range(n)]
    blob, _vk = g16.setup(ctx, g16.R1CS.from_constraints(3 * n + 1, 2, cons), *rc.TOXIC)
    rnd, zs = random.Random(11), []
    for _ in range(N):
        z = [1] + [0] * (3 * n)
        for k in range(n):
            z[1 + 3 * k], z[2 + 3 * k] = rnd.randrange(R), rnd.randrange(R)
            z[3 + 3 * k] = z[1 + 3 * k] * z[2 + 3 * k] % R
        zs.append(rc._wit(z))
    return bytes(blob), np.stack(zs)


WD_DEPTH = 2


def _wd_blob_and_records(ctx):
    """the depth-2 withdraw key's blob and N packed request records (host)"""
    from owshen_amd import circuit, groth16 as g16
    if (id(ctx), "wd-blob") not in _CACHE:
        blob, _vk = g16.setup(ctx, circuit.withdraw_r1cs(ctx.mimc7_constants(), WD_DEPTH, 0, 0), 101, 202, 303, 404, 505)
        rnd = random.Random(12)
        ins = [dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=7, recipient=9, pad_seed=rnd.randrange(R), index=rnd.randrange(4),
                    siblings=[rnd.randrange(R) for _ in range(WD_DEPTH)], token=rnd.randrange(1 << 160), chain_id=1387) for _ in range(N)]
        _CACHE[(id(ctx), "wd-blob")] = (ctx, bytes(blob), np.stack([circuit.pack_inputs(**i) for i in ins]))
    return _CACHE[(id(ctx), "wd-blob")][1:]


def _build_wd(ctx):
    from owshen_amd import circuit
    blob, recs = _wd_blob_and_records(ctx)
    wit_d = circuit.witness(ctx, WD_DEPTH, ctx.to_device(recs), 0, 0)
    return blob, np.array(ctx.to_host(wit_d), copy=True)


def _build_pc(ctx):
    from owshen_amd import groth16 as g16
    c = PcCircuit()
    blob, _vk = g16.setup(ctx, c.r1cs(), *rc.TOXIC)
    return bytes(blob), np.stack([c.witness(1300 + t) for t in range(N)])


BUILD = {"W": _build_w, "D11": _build_d11, "WD": _build_wd, "PC": _build_pc}


class Keys:
    def __init__(self, ctx, name):
        from owshen_amd import groth16 as g16
        from tests.r1cs_util import oracle_c_key_from_blob
        self.blob, self.zs = BUILD[name](ctx)
        self.rs = rc._rs(N, 1000 + len(name))
        with _env(OG_H_FORM="1"):
            self.ev = g16.ProvingKey(ctx, self.blob)
        with _env(OG_H_FORM="1", OG_MERGE_LH="0"):
            self.ev_apart = g16.ProvingKey(ctx, self.blob)       # L and H each with a bucket set of its own
        with _env(OG_H_FORM="0"):
            self.coef = g16.ProvingKey(ctx, self.blob)
        oracle = oracle_c_key_from_blob(bytes(self.blob))
        self.want = [oracle.prove(z, r, s) for z, (r, s) in zip(self.zs, self.rs)]
        assert [p.tobytes() for p in self.coef.prove_batch(self.zs, self.rs)] == self.want
        f, fc = self.ev.query_forms(), self.coef.query_forms()
        assert all(f[q]["eval"] for q in ("l", "h")) and not any(f[q]["eval"] for q in ("a", "b1", "b2")) and not any(q["eval"] for q in fc.values())
        assert f["l"]["form"] == f["h"]["form"] == "wire"                     # ("form" stays what the scalars are indexed by: wires, not rows)
        assert f["h"]["points"] == 1 << self.ev.log_d and fc["h"]["points"] == (1 << self.ev.log_d) - 1
        assert f["l"]["bits"] == f["h"]["bits"] == fc["h"]["bits"]            # the same window bits; L and H merge by default
        # og_pk_density / og_pk_windows describe the blob's own queries whatever the form
        assert self.ev.density() == self.coef.density() and self.ev.windows() == self.coef.windows()

    def same(self, got, n):
        assert [p.tobytes() for p in got] == self.want[:n]


def keys(ctx, name):
    if (id(ctx), name) not in _CACHE:
        _CACHE[(id(ctx), name)] = (ctx, Keys(ctx, name))
    return _CACHE[(id(ctx), name)][1]


# ---- 1: the same proofs, schedule by schedule ---------------------------------------------------------------------------------------
def case_fan_out(ctx, name, n):
    k = keys(ctx, name)
    assert k.ev.plan(n) == ("query fan-out", [n])
    k.same(k.ev.prove_batch(k.zs[:n], k.rs[:n]), n)
    k.same(k.ev.prove_batch_device(ctx.to_device(k.zs[:n]), k.rs[:n]), n)


def case_serial(ctx, name):
    k = keys(ctx, name)
    ctx.set_lanes(1)
    try:
        assert k.ev.plan(3)[0] == "serial"
        k.same(k.ev.prove_batch(k.zs[:3], k.rs[:3]), 3)
    finally:
        ctx.set_lanes(2)


def case_pipeline(ctx, name, monkeypatch):
    """9 proofs in sub-batches of 1, 2, 2, 2, 2 through the stage pipeline: both scratch slots reused; L and H as one
    multi-scalar multiplication and as two"""
    k = keys(ctx, name)
    monkeypatch.setenv("OG_SUB_BATCH", "2")
    monkeypatch.setenv("OG_PIPE_MIN", "1")
    for pk in (k.ev, k.ev_apart):
        assert pk.plan(N) == ("stage pipeline", [1, 2, 2, 2, 2])
        k.same(pk.prove_batch(k.zs, k.rs), N)


def case_sharded(ctx, name):
    """every rank's front half played in turn on this device, the blocks laid out as the all-gather leaves them"""
    k, world, n = keys(ctx, name), 2, 3
    zs_d = ctx.to_device(k.zs[:n])
    parts = [np.array(ctx.to_host(k.ev.prove_partials_device(zs_d, r, world)).reshape(-1), copy=True) for r in range(world)]
    k.same(k.ev.prove_from_partials(ctx.to_device(np.concatenate(parts)), world, k.rs[:n]), n)


def case_radix2(ctx, name, monkeypatch):
    k = keys(ctx, name)
    monkeypatch.setenv("OG_NTT_RADIX4", "0")
    k.same(k.ev.prove_batch(k.zs[:3], k.rs[:3]), 3)


# ---- 2: refusals and the rule ------------------------------------------------------------------------------------------------------------
def case_unsatisfied(ctx):
    """the C product and the row check stay: one bad witness in a batch is named, as before"""
    from owshen_amd.api import OwshenGpuError
    k = keys(ctx, "PC")
    zs = k.zs[:3].copy()
    zs[1, 4, 0] ^= 1                                    # a factor of constraint 0: its product is no longer public wire 1
    with pytest.raises(OwshenGpuError) as e:
        k.ev.prove_batch(zs, k.rs[:3])
    assert e.value.code == -4 and "witness 1" in str(e.value)
    k.same(k.ev.prove_batch(k.zs[:3], k.rs[:3]), 3)    # nothing is left behind


def case_flag1_key_keeps_the_old_form(ctx):
    """an imported key without a C matrix (header flag 1) has nothing to fold: forced or not, it loads and proves as before"""
    from oracle.py import zkey as zo
    from owshen_amd import groth16 as g16, zkey as zk
    from tests import zkey_cases as zc
    from tests.r1cs_util import oracle_c_key_from_blob, random_r1cs
    n_wires, cons, z0 = random_r1cs(12, 2, seed=1012, bool_every=5)
    pk_blob, _vk = zk.import_zkey(ctx, zo.write_zkey(zo.snarkjs_setup(n_wires, 2, cons, *zc._toxic(12))))
    with _env(OG_H_FORM="1"):
        pk = g16.ProvingKey(ctx, pk_blob)
    f = pk.query_forms()
    assert not f["l"]["eval"] and not f["h"]["eval"] and f["h"]["points"] == (1 << pk.log_d) - 1
    assert pk.prove(zc._wit(z0), 3, 4) == oracle_c_key_from_blob(pk_blob).prove(zc._wit(z0), 3, 4)
    pk.close()


def case_below_the_bound(ctx):
    """the rule: a C matrix and a domain of 2^14 or more.  Without the override every key here stays as it was"""
    from owshen_amd import groth16 as g16
    k = keys(ctx, "PC")
    pk = g16.ProvingKey(ctx, k.blob)
    assert pk.log_d < 14 and pk.query_forms() == k.coef.query_forms() and pk.hbm_bytes() == k.coef.hbm_bytes()
    k.same(pk.prove_batch(k.zs[:2], k.rs[:2]), 2)
    pk.close()


def case_fold_reaches_public_and_constant_wires(ctx):
    """PC's L query in the evaluation form: its own wires, and wire 0 and the two public wires with the fold of C alone as base"""
    k = keys(ctx, "PC")
    assert k.ev.query_forms()["l"]["points"] == k.ev.n_wires and k.ev.density()["l"] == k.ev.n_wires - 3


def case_corrupted_tables_are_refused(ctx, which):
    """hooks build: OG_H_FORM_CORRUPT=1 puts a wrong point into the derived H tables, 2 into the derived L tables; the load-time
    check refuses the key, and the context stays usable"""
    from owshen_amd import groth16 as g16
    from owshen_amd.api import OwshenGpuError
    k = keys(ctx, "PC")
    with _env(OG_H_FORM="1", OG_H_FORM_CORRUPT=which):
        with pytest.raises(OwshenGpuError) as e:
            g16.ProvingKey(ctx, k.blob)
    assert e.value.code == -1 and "evaluation form" in str(e.value)
    assert ("H tables" if which == "1" else "C fold") in str(e.value)
    k.same(k.ev.prove_batch(k.zs[:1], k.rs[:1]), 1)


# ---- 3: the load beside a submitted call; the pipeline's shapes; merged and unmerged ---------------------------------------------------
def case_load_is_refused_while_a_job_is_pending(ctx, load_after):
    """The load-time check of a key in the evaluation form sorts and accumulates in the context's scratch -- the scratch of a
    submitted call that has not been waited for.  Such a load is refused, the job is untouched and delivers the blocking call's
    proofs.  load_after (the GPU run, where a load takes no time): a key that stays in the coefficient form loads beside the job
    as it always did, and once the job is consumed the same blob loads in the evaluation form."""
    from owshen_amd import circuit, groth16 as g16
    from owshen_amd.api import OwshenGpuError
    blob, recs = _wd_blob_and_records(ctx)
    with _env(OG_H_FORM="0"):
        pk = g16.ProvingKey(ctx, blob)
    recs_d, rs = ctx.to_device(recs[:2]), rc._rs(2, 31)
    want = circuit.prove_from_inputs(ctx, pk, WD_DEPTH, recs_d, rs)
    job = circuit.submit_from_inputs(ctx, pk, WD_DEPTH, recs_d, rs)
    try:
        with _env(OG_H_FORM="1"):
            with pytest.raises(OwshenGpuError) as e:
                g16.ProvingKey(ctx, blob)
        assert e.value.code == -1 and "og_job_wait" in str(e.value) and "evaluation form" in str(e.value)
        if load_after:
            with _env(OG_H_FORM="0"):
                g16.ProvingKey(ctx, blob).close()
    finally:
        got = job.wait()
    assert got.tobytes() == want.tobytes()
    if load_after:
        with _env(OG_H_FORM="1"):
            ev = g16.ProvingKey(ctx, blob)
        assert ev.query_forms()["h"]["eval"]
        assert circuit.prove_from_inputs(ctx, ev, WD_DEPTH, recs_d, rs).tobytes() == want.tobytes()
        ev.close()
    pk.close()


def _ints(arr):
    return [int.from_bytes(arr[i].tobytes(), "little") for i in range(arr.shape[0])]


def case_coset_pipeline_shapes(ctx, log_d, monkeypatch):
    """The evaluation form's half of the quotient alone, without a key (hooks build: OG_H_POLY_COSET makes og_h_poly_d answer with
    it): two random polynomials per call, the coset values of their product against iNTT + coset NTT by og_ntt_fr_d and a
    product of integers.  2^5: one stage block; 2^11: two, the second a single stage; 2^12, 2^13: a second block of 2 and 3
    stages (the withdraw key's shape); with the radix-4 and the radix-2 kernel."""
    d = 1 << log_d
    rnd = random.Random(40 + log_d)
    a, b = (np.stack([rc._wit([rnd.randrange(R) for _ in range(d)]) for _ in range(2)]) for _ in range(2))
    a_d, b_d = ctx.to_device(a), ctx.to_device(b)
    ca, cb = (np.array(ctx.to_host(ctx.ntt(ctx.ntt(x, inverse=True), coset=True)), copy=True) for x in (a_d, b_d))
    want = [[x * y % R for x, y in zip(_ints(ca[g]), _ints(cb[g]))] for g in range(2)]
    monkeypatch.setenv("OG_H_POLY_COSET", "1")
    for radix4 in ("1", "0"):
        monkeypatch.setenv("OG_NTT_RADIX4", radix4)
        got = np.array(ctx.to_host(ctx.h_poly(a_d, b_d, a_d)), copy=True)
        assert [_ints(got[g]) for g in range(2)] == want, (log_d, radix4)


def case_merged_and_unmerged_differ(ctx, name):
    """`ev` runs L and H as ONE multi-scalar multiplication (one bucket reduction per proof), `ev_apart` (OG_MERGE_LH=0 at load)
    as two: seen in the reduction launches the profile counts for one serial proof -- so the two pipeline runs above are two paths"""
    k = keys(ctx, name)
    ctx.set_lanes(1)
    try:
        launches = []
        for pk in (k.ev, k.ev_apart):
            ctx.profile(True)
            k.same(pk.prove_batch(k.zs[:1], k.rs[:1]), 1)
            launches.append(ctx.profile_read()["reduce_g1"][1])
            ctx.profile(False)
    finally:
        ctx.set_lanes(2)
    assert launches[0] < launches[1], launches
