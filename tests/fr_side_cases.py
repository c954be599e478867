"""The Fr-side kernels between the transforms and the multi-scalar multiplications, each against integers of its own: the Lagrange
basis (og_lagrange_evals_d), the sparse row product (og_spmv_fr_d, and k_spmv / k_spmv_long at their 2048-entry split through a
key), the quotient's evaluation form at the inputs that maximise its lazy sums, and og_setup's refusals.  Cases shared by the
CPU-interpreter run (test_emu_fr_side.py) and the GPU run (test_gpu_fr_side.py) -- TEST INFRASTRUCTURE ONLY.

Every comparison is exact: integers mod r, or proof / key bytes.  There is no tolerance anywhere.  The expected values come from
Python integers and from the C restatement (oracle/c), never from the library's own transforms."""
import contextlib
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

from oracle.py import fields
from tests import quotient_cases as qc, row_form_cases as rc

R = fields.R
_CACHE = {}


def _bytes(vs):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vs), dtype=np.uint8).reshape(-1, 32).copy()


def _ints(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, 32).tobytes()
    return [int.from_bytes(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]


def _host(ctx, buf):
    return np.array(ctx.to_host(buf), copy=True)


@contextlib.contextmanager
def _env(**kw):
    """kw: name -> value, None to unset"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- A: the Lagrange basis ----------------------------------------------------------------------------------------------------------
LAG_SIZES = (0, 1, 2, 5, 10, 13)
LAG_TAUS = ("random", "zero", "coset generator", "one", "w^3", "w^(d-1)", "r-1")
LAG_BAD_TAUS = {"r": R, "5+r": 5 + R, "2^256-1": (1 << 256) - 1}


@functools.lru_cache(None)
def _domain(log_d):
    w, ws = fields.fr_root_of_unity(log_d), [1]
    for _ in range((1 << log_d) - 1):
        ws.append(ws[-1] * w % R)
    return tuple(ws)


def lag_tau(log_d, name):
    d, w = 1 << log_d, fields.fr_root_of_unity(log_d)
    return {"random": random.Random(7000 + log_d).randrange(R), "zero": 0, "coset generator": 7, "one": 1, "w^3": pow(w, 3 % d, R),
            "w^(d-1)": pow(w, d - 1, R), "r-1": R - 1}[name]


def lag_expected(log_d, tau):
    """off the domain (tau^d - 1)/d * w^k / (tau - w^k); at tau = w^j the unit vector e_j"""
    d, ws = 1 << log_d, _domain(log_d)
    if pow(tau, d, R) == 1:
        assert ws.count(tau) == 1
        return [int(wk == tau) for wk in ws]
    z = (pow(tau, d, R) - 1) * pow(d, -1, R) % R
    return [z * wk % R * pow(tau - wk, -1, R) % R for wk in ws]


def lag_by_product(log_d, tau):
    """the definition: prod_{i != k} (tau - w^i) / (w^k - w^i)"""
    ws, out = _domain(log_d), []
    for k, wk in enumerate(ws):
        num = den = 1
        for i, wi in enumerate(ws):
            if i != k:
                num, den = num * (tau - wi) % R, den * (wk - wi) % R
        out.append(num * pow(den, -1, R) % R)
    return out


@functools.lru_cache(None)
def _lag_poly(log_d):
    """a seeded random polynomial of degree < d and its values over the domain by the C restatement: e_k = p(w^k), natural order"""
    from oracle.c import binding as oc
    rnd = random.Random(7100 + log_d)
    p = [rnd.randrange(R) for _ in range(1 << log_d)]
    return tuple(p), tuple(_ints(oc.ntt(_bytes(p))))


def case_lagrange(ctx, log_d, name):
    tau = lag_tau(log_d, name)
    on_domain = pow(tau, 1 << log_d, R) == 1
    assert on_domain == (name in ("one", "w^3", "w^(d-1)") or (name == "r-1" and log_d >= 1))
    got = _ints(_host(ctx, ctx.lagrange_evals(log_d, tau)))
    want = lag_expected(log_d, tau)
    assert len(got) == 1 << log_d and all(v < R for v in got), "an element is not canonical"
    assert got == want
    if log_d <= 5:
        assert want == lag_by_product(log_d, tau)
    assert sum(got) % R == 1
    p, e = _lag_poly(log_d)
    at_tau = 0
    for c in reversed(p):
        at_tau = (at_tau * tau + c) % R
    assert sum(l * v for l, v in zip(got, e)) % R == at_tau       # the basis is in the natural order of the domain


def case_lagrange_refuses(ctx, name):
    from owshen_amd.api import OwshenGpuError
    with pytest.raises(OwshenGpuError) as e:
        ctx.lagrange_evals(3, LAG_BAD_TAUS[name])
    assert e.value.code == -1 and "og_lagrange_evals_d" in str(e.value), str(e.value)
    tau = lag_tau(3, "random")                                     # the context still answers
    assert _ints(_host(ctx, ctx.lagrange_evals(3, tau))) == lag_expected(3, tau)


# ---- B: og_spmv_fr_d against Python integers ------------------------------------------------------------------------------------------
SPMV_COLS = 500
SPMV_ROWS = (0, 1, 255, 256, 257, 1000)
SPMV_LONG_ROW = 3000    # one lane walks it: this entry point passes long_row = 0xffffffff, k_spmv_long is never launched


def _edge_value(rnd):
    return rnd.choice((0, 1, R - 1, rnd.randrange(R)))


def spmv_matrices(n_rows):
    """lists of row lengths: the first and the last row empty, 0 / 1 / 3 and a few more in between, one row of 3000 entries (at
    index 255 where there is one: the first lane of the second workgroup); a single row takes each length in turn"""
    if n_rows == 0:
        return [[]]
    if n_rows == 1:
        return [[0], [1], [3], [SPMV_LONG_ROW]]
    rnd = random.Random(8000 + n_rows)
    lens = [(0, 1, 3, rnd.randrange(2, 13))[rnd.randrange(4)] for _ in range(n_rows)]
    lens[0] = lens[-1] = 0
    lens[1], lens[2], lens[3] = 1, 3, 0
    lens[min(255, n_rows - 2)] = SPMV_LONG_ROW
    return [lens]


def case_spmv(ctx, n_rows):
    for t, lens in enumerate(spmv_matrices(n_rows)):
        rnd = random.Random(8100 + 10 * n_rows + t)
        x = [_edge_value(rnd) for _ in range(SPMV_COLS)]
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        col = [rnd.randrange(SPMV_COLS) for _ in range(int(ptr[-1]))]            # columns repeat inside a row
        val = [_edge_value(rnd) for _ in col]
        want = [sum(val[k] * x[col[k]] for k in range(ptr[i], ptr[i + 1])) % R for i in range(n_rows)]
        val_np = _bytes(val) if val else np.zeros((0, 32), np.uint8)
        got = ctx.spmv(ctx.to_device(ptr), ctx.to_device(np.array(col, dtype=np.uint32)), ctx.to_device(val_np), ctx.to_device(_bytes(x)), n_rows)
        got = _ints(_host(ctx, got))
        assert len(got) == n_rows and all(v < R for v in got), "an element is not canonical"
        assert got == want, (n_rows, lens[:4])
        if SPMV_LONG_ROW in lens:
            i = lens.index(SPMV_LONG_ROW)
            assert len(set(col[ptr[i]:ptr[i + 1]])) < SPMV_LONG_ROW                 # (3000 draws from 500 columns)


# ---- C: the row product at its 2048-entry split, through a key ----------------------------------------------------------------------
class BoundaryCircuit:
    """7 constraints over 2 public wires, a pool of 2400 shared wires and one fresh wire per constraint (C coefficient 1: whatever
    the pool holds, the fresh wires complete the witness).  Entries per row, pool wires unless said otherwise:
        k   A                          B                      C
        0   2047                       2                      2048 + the fresh wire = 2049
        1   2048                       1                      the fresh wire
        2   2047 + TAIL[0] = 2049      3                      "
        3   2304                       2                      "
        4   2304 + TAIL[1] = 2305      2049                   "
        5   3 (two public wires)       2049                   "
        6   2 (one public wire)        2048                   "
    Rows of MORE than 2048 entries go to k_spmv_long, a workgroup each; 2047 and 2048 stay on one lane of k_spmv.  2049 and 2305
    are 256 q + 1: the last entry is the one step of the strided loop that thread 0 alone takes.  TAIL[0] / TAIL[1] are the two
    highest pool wires and occur in no other row, so -- entries being sorted by wire -- each is the LAST entry of its row."""
    N_PUB, POOL = 2, 2400
    A_LENS = (2047, 2048, 2049, 2304, 2305)

    def __init__(self):
        rnd = random.Random(9000)
        first = 1 + self.N_PUB
        self.pool = range(first, first + self.POOL)
        self.tail = (first + self.POOL - 2, first + self.POOL - 1)
        shared = list(self.pool)[:-2]

        def coeff():
            return rnd.choice((1, R - 1, rnd.randrange(1, R)))

        def row(n, extra=()):
            return {w: coeff() for w in list(extra) + rnd.sample(shared, n - len(extra))}

        a = [row(2047), row(2048), row(2049, [self.tail[0]]), row(2304), row(2305, [self.tail[1]]), row(3, [1, 2]), row(2, [2])]
        b = [row(2), row(1), row(3), row(2), row(2049), row(2049), row(2048)]
        self.fresh = [first + self.POOL + k for k in range(7)]
        c = [{self.fresh[k]: 1} for k in range(7)]
        c[0].update(row(2048))
        self.cons = list(zip(a, b, c))
        self.n_wires = first + self.POOL + 7
        assert [len(x) for x in a[:5]] == list(self.A_LENS) and [len(x) for x in b[4:]] == [2049, 2049, 2048] and len(c[0]) == 2049
        for t, k in zip(self.tail, (2, 4)):
            assert max(a[k]) == t and sum(t in lc for con in self.cons for lc in con) == 1

    def r1cs(self):
        from owshen_amd import groth16 as g16
        return g16.R1CS.from_constraints(self.n_wires, self.N_PUB, self.cons)

    def witness(self, seed):
        rnd = random.Random(seed)
        z = [1] + [rnd.randrange(R) for _ in range(self.N_PUB)] + [_edge_value(rnd) for _ in self.pool] + [0] * 7
        for k, (a, b, c) in enumerate(self.cons):
            dot = lambda lc: sum(v * z[w] for w, v in lc.items()) % R
            z[self.fresh[k]] = (dot(a) * dot(b) - dot(c)) % R       # (the fresh wire is still 0 in dot(c))
            assert dot(a) * dot(b) % R == dot(c)
            if k in (2, 4):
                assert dot(b) != 0                                     # a change of A z in this row cannot go unseen
        return z


class BoundaryKey:
    def __init__(self, ctx):
        from owshen_amd import groth16 as g16
        from tests.r1cs_util import oracle_c_key_from_blob
        self.circuit = BoundaryCircuit()
        self.blob, _vk = g16.setup(ctx, self.circuit.r1cs(), *rc.TOXIC)
        assert self.blob.rows is not None
        self.row = g16.ProvingKey(ctx, self.blob)
        self.plain = g16.ProvingKey(ctx, bytes(self.blob))
        self.z = [self.circuit.witness(9100 + t) for t in range(4)]
        self.zs = np.stack([_bytes(z) for z in self.z])
        self.rs = rc._rs(4, 91)
        oracle = oracle_c_key_from_blob(bytes(self.blob))
        self.want = [oracle.prove(w, r, s) for w, (r, s) in zip(self.zs, self.rs)]


def boundary_key(ctx):
    if (id(ctx), "boundary") not in _CACHE:
        _CACHE[(id(ctx), "boundary")] = (ctx, BoundaryKey(ctx))
    return _CACHE[(id(ctx), "boundary")][1]


def case_boundary_forms(ctx):
    """the key takes A and B over the rows, so the canonical copy that k_spmv_long leaves is what feeds those sums"""
    k = boundary_key(ctx)
    f = k.row.query_forms()
    assert [f[q]["form"] for q in ("a", "b1", "b2", "l", "h")] == ["row", "row", "row", "wire", "wire"], f
    assert all(q["form"] == "wire" for q in k.plain.query_forms().values())
    assert (k.row.n_wires, k.row.n_pub, k.row.log_d, k.row.n_rows) == (k.circuit.n_wires, 2, 4, 10)


def case_boundary_proofs(ctx):
    """three witnesses in one call (blockIdx.y of k_spmv_long, the stride of the canonical copy), then one alone"""
    k = boundary_key(ctx)
    for pk in (k.row, k.plain):
        assert [p.tobytes() for p in pk.prove_batch(k.zs[:3], k.rs[:3])] == k.want[:3]
        assert [p.tobytes() for p in pk.prove_batch(k.zs[3:], k.rs[3:])] == k.want[3:]


def case_boundary_unsatisfied(ctx, which):
    """a wire that only the LAST entry of a long A row reads, changed in witness 1 of 3"""
    from owshen_amd.api import OwshenGpuError
    k = boundary_key(ctx)
    wire = k.circuit.tail[which]
    for pk in (k.row, k.plain):
        zs = k.zs[:3].copy()
        zs[1, wire] = _bytes([(k.z[1][wire] + 1) % R])[0]
        with pytest.raises(OwshenGpuError) as e:
            pk.prove_batch(zs, k.rs[:3])
        assert e.value.code == -4 and "witness 1" in str(e.value), str(e.value)
        assert [p.tobytes() for p in pk.prove_batch(k.zs[:3], k.rs[:3])] == k.want[:3]       # nothing is left behind


def case_boundary_eval_form(ctx):
    """hooks build, OG_H_FORM=1: C folded into L, C z -- its 2049-entry row on k_spmv_long -- still computed for the row check"""
    from owshen_amd import groth16 as g16
    from owshen_amd.api import OwshenGpuError
    k = boundary_key(ctx)
    with _env(OG_H_FORM="1"):
        ev = g16.ProvingKey(ctx, k.blob)
    try:
        f = ev.query_forms()
        assert f["l"]["eval"] and f["h"]["eval"] and [f[q]["form"] for q in ("a", "b1", "b2")] == ["row"] * 3, f
        assert [p.tobytes() for p in ev.prove_batch(k.zs[:3], k.rs[:3])] == k.want[:3]
        zs = k.zs[:3].copy()
        zs[1, k.circuit.fresh[0]] = _bytes([(k.z[1][k.circuit.fresh[0]] + 1) % R])[0]       # read by the 2049-entry C row alone
        with pytest.raises(OwshenGpuError) as e:
            ev.prove_batch(zs, k.rs[:3])
        assert e.value.code == -4 and "witness 1" in str(e.value), str(e.value)
    finally:
        ev.close()


# ---- D: the evaluation form of the quotient at its bounds ---------------------------------------------------------------------------
@functools.lru_cache(None)
def _coset_values(key):
    """the C restatement's values over the coset of the polynomial with the given values over the domain; each distinct input once"""
    from oracle.c import binding as oc
    x = np.frombuffer(key, dtype=np.uint8).reshape(-1, 32)
    return tuple(_ints(oc.ntt(oc.ntt(x, inverse=True), coset=True)))


def _coset_product(a, b):
    ca, cb = _coset_values(a.tobytes()), _coset_values(b.tobytes())
    return b"".join((x * y % R).to_bytes(32, "little") for x, y in zip(ca, cb))


def _run_coset(ctx, pairs, third, label):
    """pairs: (a, b) per batch item -- the rows differ, so an item that read another's pw_a would show.  Radix-4 and radix-2 kernel."""
    a_d, b_d = (ctx.to_device(np.stack([p[i] for p in pairs])) for i in (0, 1))
    c_d = ctx.to_device(np.stack([third] * len(pairs)))                        # ignored by this form
    want = [_coset_product(a, b) for a, b in pairs]
    for radix4 in (None, "0"):
        with _env(OG_H_POLY_COSET="1", OG_NTT_RADIX4=radix4):
            got = _host(ctx, ctx.h_poly(a_d, b_d, c_d))
        for g in range(len(pairs)):
            assert got[g].tobytes() == want[g], (label, "item", g, "OG_NTT_RADIX4", radix4)


def case_coset_extremes(ctx, log_d):
    """the four triples that maximise every lazy sum of k_ntt_block4, in batches of two: each triple once as item 0, once as item 1"""
    ts = qc.extreme_triples(1 << log_d)
    for k in range(4):
        (a0, b0, c0), (a1, b1, _c1) = ts[k], ts[(k + 1) % 4]
        _run_coset(ctx, [(a0, b0), (a1, b1)], c0, (log_d, "triples", k, (k + 1) % 4))


def case_coset_block_shapes(ctx, log_d):
    a, b, c = qc.block_shape_inputs(log_d)
    _run_coset(ctx, [(a, b), (c, a)], c, (log_d, "block shape inputs"))


# ---- E: og_setup refuses bad toxic values ---------------------------------------------------------------------------------------------
def _raw_setup(ctx, r1cs, toxic):
    """og_setup with the five values as given (owshen_amd.groth16.setup asserts 0 < v < r before the library sees them)"""
    from owshen_amd import groth16 as g16
    lib = ctx._lib
    rc_, h, _keep = g16._r1cs_handle(lib, r1cs)
    ctx._check(rc_)
    try:
        buf = (C.c_uint8 * 160).from_buffer_copy(b"".join(int(v).to_bytes(32, "little") for v in toxic))
        pk_p, vk_p, pk_n, vk_n = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        ctx._pre()
        try:
            ctx._check(lib.og_setup(ctx._h, h, buf, C.byref(pk_p), C.byref(pk_n), C.byref(vk_p), C.byref(vk_n)))
            return C.string_at(pk_p, pk_n.value), C.string_at(vk_p, vk_n.value)
        finally:
            lib.og_blob_free(pk_p)
            lib.og_blob_free(vk_p)
    finally:
        lib.og_r1cs_free(h)


def case_setup_refusals(ctx):
    from owshen_amd import groth16 as g16
    from owshen_amd.api import OwshenGpuError
    r1 = rc.Circuit(8, 8).r1cs()
    assert r1.log_d == 5
    before, _vk = g16.setup(ctx, r1, *rc.TOXIC)
    assert _raw_setup(ctx, r1, rc.TOXIC)[0] == bytes(before)                    # the raw call is the same call
    w = fields.fr_root_of_unity(5)
    bad = [((tau,) + rc.TOXIC[1:], "evaluation domain") for tau in (1, pow(w, 5, R), R - 1)]
    bad += [(rc.TOXIC[:k] + (0,) + rc.TOXIC[k + 1:], "canonical and non-zero") for k in range(5)]
    bad += [(rc.TOXIC[:1] + (R,) + rc.TOXIC[2:], "canonical and non-zero"), (rc.TOXIC[:4] + ((1 << 256) - 1,), "canonical and non-zero")]
    for toxic, words in bad:
        with pytest.raises(OwshenGpuError) as e:
            _raw_setup(ctx, r1, toxic)
        assert e.value.code == -1 and words in str(e.value), (toxic, str(e.value))
    after, _vk = g16.setup(ctx, r1, *rc.TOXIC)
    assert bytes(after) == bytes(before) and after.rows == before.rows and before.rows is not None
