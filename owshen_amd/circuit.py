"""The withdraw circuit as an R1CS, plus input packing for the GPU witness generator.

No reference counterpart: the snapshot's withdraw is an ECDSA-authorised burn
(/root/reference/src/services/api_services/withdraw.rs:27-71) with no circuit.
The statement is

    public : root, nullifier_hash, recipient, amount, token, chain_id
    private: nullifier, secret, Merkle path (siblings, index) of depth D
    leaf = H(H(nullifier, secret), H(amount, token)) lies under root;  nullifier_hash = H(nullifier, 0)

with H = MultiMiMC7 (circomlib convention).  The six public inputs cover what the reference's ECDSA gate signs
(/root/reference/contracts/src/Owshen.sol:69: msg.sender, token, amount, id, chainid -- the nullifier hash stands in for
the replay id); the token sits inside the leaf, which the ledger forms at deposit time from the depositor's inner
commitment H(nullifier, secret) and the asset it actually credited (oracle/py/withdraw.py).  Wire and constraint order are a contract shared
with owshen_amd/csrc/witness.hip (which fills the wires on the GPU); tests check both against
the plain restatement in oracle/py/withdraw.py.  `n_pad3` / `n_pad2` append synthetic
multiplication gates that size the statement to BASELINE.json's configs[1] ("MSM ~2^20 G1
points, Fr NTT 2^17"): n_wires = 2^18, domain 2^17.

Only index arrays and constants are produced here (numpy); there is no host-side witness
generator -- the witness comes from og_withdraw_witness_d.

The deposit, the split, the join, the transfer, the claim, the send and the redeem statement (oracle/py/deposit.py, tests/split_spec.py,
tests/join_spec.py, tests/transfer_spec.py, tests/claim_spec.py, tests/send_spec.py, tests/redeem_spec.py are their specs) follow further
down, built with the same gadget builder.
"""
import ctypes as C

import numpy as np

from .api import FR_MODULUS as R
from .groth16 import R1CS, SparseMatrix

N_PUB = 6
N_ROUNDS = 91
PAD_SEGMENT = 64
N_DENSE_ROWS = 2
W_ROOT, W_NH, W_RECIPIENT, W_AMOUNT, W_TOKEN, W_CHAIN, W_NULLIFIER, W_SECRET = 1, 2, 3, 4, 5, 6, 7, 8
N_REC = 8  # fields of an input record before the siblings
# BabyJubJub: a x^2 + y^2 = 1 + d x^2 y^2 over Fr, its base point and l, the prime order of BASE (8 l points on the curve)
ED_A, ED_D = 168700, 168696
ED_BASE = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
           16950150798460657717958625567821834550301663161624707787222815936182638968203)
ED_L = 2736030358979909402780800718157159386076813972158567259200215660948447373041


def _ed_double(p):
    """2 p on BabyJubJub, affine (the complete law with both operands p)"""
    x, y = p
    t = ED_D * x * x % R * y * y % R
    return 2 * x * y * pow(1 + t, -1, R) % R, (y * y - ED_A * x * x) * pow(1 - t, -1, R) % R


def shape(depth, n_pad3=0, n_pad2=0):
    """(n_wires, n_constraints)"""
    hashes = 4 + depth
    pad_base = 1 + N_PUB + 2 + 2 * depth + 2 + depth + hashes * 730 - 2
    return pad_base + 3 * n_pad3 + 2 * n_pad2, 2 + 2 * depth + hashes * 730 + n_pad3 + n_pad2


def pad_for(depth, n_wires, n_constraints):
    """(n_pad3, n_pad2) that hit exactly n_wires wires and n_constraints constraints."""
    w0, c0 = shape(depth)
    p, w = n_constraints - c0, n_wires - w0
    x = w - 2 * p
    if not 0 <= x <= p:
        raise ValueError("shape not reachable with 2- and 3-wire padding gates")
    return x, p - x


def baseline_shape(depth=32, dense=False):
    """BASELINE.json configs[1]: 2^18 wires, 2^17-point domain (constraints + n_pub + 1 = 2^17).  `dense` leaves room
    for the two density rows of withdraw_r1cs(dense=True)."""
    return pad_for(depth, 1 << 18, (1 << 17) - N_PUB - 1 - (N_DENSE_ROWS if dense else 0))


class _Triplets:
    """one matrix: entries appended row by row"""

    def __init__(self):
        self.counts, self.cols, self.vals = [], [], []

    def row(self, lc):
        n = 0
        for w, c in lc:
            if c % R:
                self.cols.append(w)
                self.vals.append(c % R)
                n += 1
        self.counts.append(n)


def _lc_merge(*lcs):
    out = {}
    for lc in lcs:
        for w, c in lc:
            out[w] = (out.get(w, 0) + c) % R
    return [(w, c) for w, c in out.items() if c]


class _Builder:
    def __init__(self, consts):
        self.a, self.b, self.c = _Triplets(), _Triplets(), _Triplets()
        self.next = 0
        self.consts = consts

    def alloc(self, n=1):
        w = self.next
        self.next += n
        return w

    def enforce(self, a, b, c):
        self.a.row(a)
        self.b.row(b)
        self.c.row(c)

    def perm(self, x_lc, k_lc):
        cur = x_lc
        for i in range(N_ROUNDS):
            t = _lc_merge(cur, k_lc, [(0, self.consts[i])])
            t2 = self.alloc(4)
            t4, t6, t7 = t2 + 1, t2 + 2, t2 + 3
            self.enforce(t, t, [(t2, 1)])
            self.enforce([(t2, 1)], [(t2, 1)], [(t4, 1)])
            self.enforce([(t4, 1)], [(t2, 1)], [(t6, 1)])
            self.enforce([(t6, 1)], t, [(t7, 1)])
            cur = [(t7, 1)]
        return cur

    def hash2(self, l_lc, r_lc, out_wire=None):
        x91 = self.perm(l_lc, [])
        k1 = self.alloc()
        self.enforce(_lc_merge(l_lc, x91), [(0, 1)], [(k1, 1)])
        y91 = self.perm(r_lc, [(k1, 1)])
        if out_wire is None:
            out_wire = self.alloc()
        self.enforce(_lc_merge([(k1, 2)], r_lc, y91), [(0, 1)], [(out_wire, 1)])
        return out_wire

    def range_check(self, value, bits, n_bits=128):
        """value < 2^n_bits: boolean rows over the wires bits .. bits + n_bits - 1 (LSB first), then the recomposition row"""
        for i in range(n_bits):
            self.enforce([(bits + i, 1)], [(bits + i, 1), (0, R - 1)], [])
        self.enforce([(bits + i, 1 << i) for i in range(n_bits)], [(0, 1)], [(value, 1)])

    def less_equal_const(self, bits, n_bits, m):
        """sum 2^i b_i <= m for the constant m < 2^n_bits, over the boolean wires bits .. bits + n_bits - 1 (LSB first), most
        significant bit first: t starts as the constant 1; a 1-bit of m allocates t' = t b_i (one row), a 0-bit adds the row
        b_i t = 0.  popcount(m) wires, n_bits rows; the caller makes the wires boolean"""
        assert 0 <= m < (1 << n_bits)
        t = [(0, 1)]
        for i in reversed(range(n_bits)):
            if (m >> i) & 1:
                nt = self.alloc()
                self.enforce(t, [(bits + i, 1)], [(nt, 1)])
                t = [(nt, 1)]
            else:
                self.enforce([(bits + i, 1)], t, [])

    def fixed_base_mul(self, bits, n_bits):
        """P = (sum 2^i b_i) BASE on BabyJubJub over the wires bits .. bits + n_bits - 1 (LSB first), which it makes boolean.  Per bit
        the wires w1 = b x1, w2 = b y1, w3 = w1 y1, x3, y3 and six rows: the complete twisted Edwards law with the addend
        (b u_i, 1 + b (v_i - 1)), (u_i, v_i) = 2^i BASE, on the running sum (x1, y1) that starts at the constants (0, 1).  Returns the
        linear combinations of P.x and P.y"""
        x1, y1 = [], [(0, 1)]
        u, v = ED_BASE
        for i in range(n_bits):
            b = bits + i
            duv = ED_D * u % R * v % R
            w1 = self.alloc(5)
            w2, w3, x3, y3 = w1 + 1, w1 + 2, w1 + 3, w1 + 4
            self.enforce([(b, 1)], [(b, 1), (0, R - 1)], [])
            self.enforce([(b, 1)], x1, [(w1, 1)])
            self.enforce([(b, 1)], y1, [(w2, 1)])
            self.enforce([(w1, 1)], y1, [(w3, 1)])
            self.enforce([(x3, 1)], [(0, 1), (w3, duv)], _lc_merge(x1, [(w1, v - 1)], [(w2, u)]))
            self.enforce([(y3, 1)], [(0, 1), (w3, R - duv)], _lc_merge(y1, [(w2, v - 1)], [(w1, R - ED_A * u % R)]))
            x1, y1 = [(x3, 1)], [(y3, 1)]
            u, v = _ed_double((u, v))
        return x1, y1

    def merkle_walk(self, cur, w_sib, w_bit, depth, root):
        """the path from `cur` up to the wire `root`, the output wire of the last level's hash: per level a boolean index bit, the
        `left` selector wire (allocated here) and one hash"""
        for l in range(depth):
            b, s = w_bit + l, w_sib + l
            self.enforce([(b, 1)], [(b, 1), (0, R - 1)], [])
            left = self.alloc()
            self.enforce([(b, 1)], [(s, 1), (cur, R - 1)], [(left, 1), (cur, R - 1)])
            right = [(s, 1), (cur, 1), (left, R - 1)]
            cur = self.hash2([(left, 1)], right, out_wire=root if l == depth - 1 else None)

    def spend_note(self, nullifier, secret, amount, token, nh, w_sib, w_bit, depth, root):
        """a note is spent: leaf = H(H(nullifier, secret), H(amount, token)), nullifier_hash = H(nullifier, 0) into the wire `nh`,
        then the leaf's path up to `root`"""
        inner = self.hash2([(nullifier, 1)], [(secret, 1)])
        asset = self.hash2([(amount, 1)], [(token, 1)])
        leaf = self.hash2([(inner, 1)], [(asset, 1)])
        self.hash2([(nullifier, 1)], [], out_wire=nh)
        self.merkle_walk(leaf, w_sib, w_bit, depth, root)


def _csr(trip, pad_counts, pad_cols, pad_vals, n_wires):
    counts = np.concatenate([np.asarray(trip.counts, dtype=np.int64), pad_counts])
    ptr = np.zeros(counts.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    cols = np.concatenate([np.asarray(trip.cols, dtype=np.uint32), pad_cols.astype(np.uint32)])
    vals = list(trip.vals)
    uniq = {}
    idx = np.empty(len(vals) + pad_vals.shape[0], dtype=np.int64)
    for i, v in enumerate(vals):
        idx[i] = uniq.setdefault(v, len(uniq))
    for small in (1, 2, 3):
        uniq.setdefault(small, len(uniq))
    lut = np.zeros(4, dtype=np.int64)
    for small in (1, 2, 3):
        lut[small] = uniq[small]
    idx[len(vals):] = lut[pad_vals]
    table = np.zeros((len(uniq), 32), dtype=np.uint8)
    for v, k in uniq.items():
        table[k] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    return SparseMatrix(ptr.astype(np.uint32), cols, table[idx], n_wires)


def _pad_arrays(pad_base, n_pad3, n_pad2):
    """index arrays of the padding gates: per matrix (counts, cols, small-int values)"""
    g3 = np.arange(n_pad3, dtype=np.int64)
    p3, q3, w3 = pad_base + 3 * g3, pad_base + 3 * g3 + 1, pad_base + 3 * g3 + 2
    g2 = np.arange(n_pad2, dtype=np.int64)
    base2 = pad_base + 3 * n_pad3
    p2, w2 = base2 + 2 * g2, base2 + 2 * g2 + 1
    first = (g2 % PAD_SEGMENT) == 0
    zeros3, zeros2 = np.zeros(n_pad3, dtype=np.int64), np.zeros(n_pad2, dtype=np.int64)
    # A rows: (p, 1), (one, 1)
    a_counts = np.full(n_pad3 + n_pad2, 2, dtype=np.int64)
    a_cols = np.concatenate([np.stack([p3, zeros3], 1).ravel(), np.stack([p2, zeros2], 1).ravel()])
    a_vals = np.ones(a_cols.shape[0], dtype=np.int64)
    # B rows: 3-wire gate (q, 1), (one, 2); chained gate (prev, 1), (one, 2) or (one, 3) at a segment start
    b3_cols = np.stack([q3, zeros3], 1).ravel()
    b3_vals = np.tile(np.array([1, 2], dtype=np.int64), n_pad3)
    b2_counts = np.where(first, 1, 2)
    prev = w2 - 2
    b2_cols = np.stack([prev, zeros2], 1)
    b2_vals = np.tile(np.array([1, 2], dtype=np.int64), (n_pad2, 1))
    keep = np.ones((n_pad2, 2), dtype=bool)
    keep[first, 0] = False
    b2_vals[first, 1] = 3
    b_counts = np.concatenate([np.full(n_pad3, 2, dtype=np.int64), b2_counts])
    b_cols = np.concatenate([b3_cols, b2_cols[keep]])
    b_vals = np.concatenate([b3_vals, b2_vals[keep]])
    # C rows: (w, 1)
    c_counts = np.ones(n_pad3 + n_pad2, dtype=np.int64)
    c_cols = np.concatenate([w3, w2])
    c_vals = np.ones(c_cols.shape[0], dtype=np.int64)
    return (a_counts, a_cols, a_vals), (b_counts, b_cols, b_vals), (c_counts, c_cols, c_vals)


def withdraw_r1cs(mimc7_constants, depth=32, n_pad3=0, n_pad2=0, dense=False):
    """mimc7_constants: the 91 round constants (ints), e.g. Context.mimc7_constants().  Returns R1CS.

    dense=True appends two "density rows" after the padding gates -- (sum of all wires) * 0 = 0 and
    0 * (sum of all wires) = 0 -- which any witness satisfies (the witness generator is unchanged) but which give
    EVERY wire a non-zero A and B polynomial: the A, B1 and B2 queries then keep all n_wires bases (the worst case
    of a circuit whose wires all occur on both sides: G1 MSMs over m, m, m - 5 and d - 1 points, G2 over m), instead
    of the ~50 % / ~45 % the padding gates alone give (a wire p that only ever sits on the A side has no B base)."""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = shape(depth, n_pad3, n_pad2)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + N_PUB + 2)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_rsq = bld.alloc()
    w_csq = bld.alloc()
    bld.enforce([(W_RECIPIENT, 1)], [(W_RECIPIENT, 1)], [(w_rsq, 1)])
    bld.enforce([(W_CHAIN, 1)], [(W_CHAIN, 1)], [(w_csq, 1)])
    bld.spend_note(W_NULLIFIER, W_SECRET, W_AMOUNT, W_TOKEN, W_NH, w_sib, w_bit, depth, W_ROOT)
    pad_base = bld.next
    assert pad_base + 3 * n_pad3 + 2 * n_pad2 == n_wires
    pa, pb, pc = _pad_arrays(pad_base, n_pad3, n_pad2)
    if dense:
        allw = np.arange(n_wires, dtype=np.int64)
        none = np.zeros(0, dtype=np.int64)
        ones = np.ones(n_wires, dtype=np.int64)
        # row 1: A = all wires, B = C = 0;  row 2: B = all wires, A = C = 0
        pa = (np.concatenate([pa[0], [n_wires, 0]]), np.concatenate([pa[1], allw]), np.concatenate([pa[2], ones]))
        pb = (np.concatenate([pb[0], [0, n_wires]]), np.concatenate([pb[1], allw]), np.concatenate([pb[2], ones]))
        pc = (np.concatenate([pc[0], [0, 0]]), np.concatenate([pc[1], none]), np.concatenate([pc[2], none]))
        n_constraints += N_DENSE_ROWS
    r1cs = R1CS(n_wires, N_PUB, _csr(bld.a, *pa, n_wires), _csr(bld.b, *pb, n_wires), _csr(bld.c, *pc, n_wires))
    assert r1cs.n_constraints == n_constraints
    return r1cs


def withdraw_r1cs_native(ctx, depth=32, n_pad3=0, n_pad2=0, dense=False):
    """The same circuit built by the library (og_withdraw_r1cs -- what a Rust host calls; tests check it row by row
    against `withdraw_r1cs` and the spec).  Returns R1CS."""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_withdraw_r1cs(ctx._h, depth, n_pad3, n_pad2, int(dense), C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def _r1cs_from_handle(ctx, h):
    """og_r1cs handle -> R1CS (exports the three matrices, frees the handle)"""
    lib = ctx._lib
    try:
        info = (C.c_uint64 * 6)()
        ctx._check(lib.og_r1cs_info(h, info))
        n_wires, n_pub, nc = int(info[0]), int(info[1]), int(info[2])
        mats = []
        for k in range(3):
            nnz = int(info[3 + k])
            ptr = np.zeros(nc + 1, dtype=np.uint32)
            col = np.zeros(nnz, dtype=np.uint32)
            val = np.zeros((nnz, 32), dtype=np.uint8)
            ctx._check(lib.og_r1cs_export(h, k, ptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                          val.ctypes.data_as(C.c_void_p)))
            mats.append(SparseMatrix(ptr, col, val, n_wires))
    finally:
        lib.og_r1cs_free(h)
    return R1CS(n_wires, n_pub, *mats)


def _finish(bld, n_wires, n_pub, n_constraints):
    """the R1CS of a statement without padding gates, from its finished builder"""
    assert bld.next == n_wires
    none = np.zeros(0, dtype=np.int64)
    pad = (none, none, none)
    r1cs = R1CS(n_wires, n_pub, _csr(bld.a, *pad, n_wires), _csr(bld.b, *pad, n_wires), _csr(bld.c, *pad, n_wires))
    assert r1cs.n_constraints == n_constraints
    return r1cs


def _pack(vals):
    """field elements -> uint8 [len, 32], canonical little-endian: one input record"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _dev(ctx, *values):
    """field elements -> device uint8 [len, 32]"""
    return ctx.to_device(_pack(values))


def _records_witness(ctx, name, n_rec_fields, depth, inputs_d, shape, n_pub):
    """og_<name>_witness_d of a record statement: inputs_d device uint8 [n, n_rec_fields, 32] -> device uint8 [n, n_wires, 32]; `shape`,
    `n_pub`: what this module says of the statement, checked against og_<name>_shape"""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (n_rec_fields, 32)
    shp = (C.c_uint64 * 3)()
    ctx._check(getattr(ctx._lib, f"og_{name}_shape")(depth, shp))
    assert (int(shp[0]), int(shp[1]), int(shp[2])) == (*shape, n_pub), f"circuit.py and witness.hip disagree on the {name} shape"
    out = ctx.empty(n, int(shp[0]), 32)
    ctx._pre()
    ctx._check(getattr(ctx._lib, f"og_{name}_witness_d")(ctx._h, depth, ctx.ptr(inputs_d), n, ctx.ptr(out)))
    return out


def _records_prove(ctx, pk, name, n_rec_fields, n_pub, depth, inputs_d, rs, return_public):
    """og_<name>_prove_batch_d of a record statement -> np.uint8 [n, 256], and the public inputs np.uint8 [n, n_pub, 32] when asked for"""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (n_rec_fields, 32)
    rsb = pk._rs_bytes(rs)
    assert rsb.shape[0] == n
    out = np.zeros((n, 256), dtype=np.uint8)
    pub = np.zeros((n, n_pub, 32), dtype=np.uint8) if return_public else None
    ctx._pre()
    ctx._check(getattr(ctx._lib, f"og_{name}_prove_batch_d")(ctx._h, pk._h, depth, ctx.ptr(inputs_d), n, rsb.ctypes.data_as(C.c_void_p),
                                                            out.ctypes.data_as(C.c_void_p),
                                                            pub.ctypes.data_as(C.c_void_p) if return_public else None))
    return (out, pub) if return_public else out


def pack_inputs(nullifier, secret, amount, recipient, pad_seed, index, siblings, token=0, chain_id=0):
    """one witness-generator input record: (8 + depth) x 32 B (include/owshen_gpu.h):
    nullifier | secret | amount | recipient | pad_seed | index | token | chain_id | siblings[depth]"""
    return _pack([nullifier, secret, amount, recipient, pad_seed, index, token, chain_id] + list(siblings))


def witness(ctx, depth, inputs_d, n_pad3=0, n_pad2=0, out=None):
    """inputs_d: device uint8 [n, 8 + depth, 32] -> device uint8 [n, n_wires, 32] (og_withdraw_witness_d).
    `out`: optional preallocated device buffer of that shape."""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (N_REC + depth, 32)
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_withdraw_shape(depth, n_pad3, n_pad2, shp))
    assert (int(shp[0]), int(shp[1])) == shape(depth, n_pad3, n_pad2), "circuit.py and witness.hip disagree on the shape"
    if out is None:
        out = ctx.empty(n, int(shp[0]), 32)
    assert tuple(out.shape) == (n, int(shp[0]), 32)
    ctx._pre()
    ctx._check(ctx._lib.og_withdraw_witness_d(ctx._h, depth, n_pad3, n_pad2, ctx.ptr(inputs_d), n, ctx.ptr(out)))
    return out


def prove_from_inputs(ctx, pk, depth, inputs_d, rs, n_pad3=0, n_pad2=0, return_public=False):
    """inputs_d: device uint8 [n, 8 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256]
    (og_withdraw_prove_batch_d: witness generation fused into the prover's lanes).  return_public: also the public inputs
    of every proof (root, nullifier_hash, recipient, amount, token, chain_id), np.uint8 [n, 6, 32]."""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (N_REC + depth, 32)
    rsb = pk._rs_bytes(rs)
    assert rsb.shape[0] == n
    out = np.zeros((n, 256), dtype=np.uint8)
    pub = np.zeros((n, N_PUB, 32), dtype=np.uint8) if return_public else None
    ctx._pre()
    ctx._check(ctx._lib.og_withdraw_prove_batch_d(ctx._h, pk._h, depth, n_pad3, n_pad2, ctx.ptr(inputs_d), n,
                                                  rsb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                  pub.ctypes.data_as(C.c_void_p) if return_public else None))
    return (out, pub) if return_public else out


def partials_from_inputs(ctx, pk, depth, inputs_d, win_rank, win_world, n_pad3=0, n_pad2=0, return_public=False):
    """The front half of a window-sharded call on this rank (og_withdraw_prove_partials_d): inputs_d device uint8
    [n, 8 + depth, 32] -> device uint8 [n * 768], this rank's partial points of the five queries (windows k = win_rank mod
    win_world); return_public: also the public inputs np.uint8 [n, 6, 32].  owshen_amd/shard.py composes it with the all-gather
    and ProvingKey.prove_from_partials."""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (N_REC + depth, 32)
    part = ctx.empty(n * pk.PARTIAL_BYTES)
    pub = np.zeros((n, N_PUB, 32), dtype=np.uint8) if return_public else None
    ctx._pre()
    ctx._check(ctx._lib.og_withdraw_prove_partials_d(ctx._h, pk._h, depth, n_pad3, n_pad2, ctx.ptr(inputs_d), n, win_rank, win_world,
                                                     ctx.ptr(part), pub.ctypes.data_as(C.c_void_p) if return_public else None))
    return (part, pub) if return_public else part


# ---- the deposit statement (oracle/py/deposit.py is the spec; witness.hip k_deposit_witness fills the wires) ----------------
# public: commitment, depositor; private: nullifier, secret; commitment = H(nullifier, secret); depositor bound by its square.
# The reference's deposit (/root/reference/src/services/api_services/deposit.rs:32-154 -> mint_tx.rs:11-49) has no commitment
# and no proof; with notes the ledger refuses a commitment nobody can open (og_verify with (c, DepositRequest.address)).
D_N_PUB, D_N_REC = 2, 3
DW_COMMITMENT, DW_DEPOSITOR, DW_NULLIFIER, DW_SECRET = 1, 2, 3, 4


def deposit_shape():
    """(n_wires, n_constraints) = (735, 731)"""
    return 6 + 729, 1 + 730


def deposit_r1cs(mimc7_constants):
    """the deposit statement as an R1CS (the same gadget builder as the withdraw circuit)"""
    assert len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = deposit_shape()
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + D_N_PUB + 2)
    w_dsq = bld.alloc()
    bld.enforce([(DW_DEPOSITOR, 1)], [(DW_DEPOSITOR, 1)], [(w_dsq, 1)])
    bld.hash2([(DW_NULLIFIER, 1)], [(DW_SECRET, 1)], out_wire=DW_COMMITMENT)
    return _finish(bld, n_wires, D_N_PUB, n_constraints)


def deposit_r1cs_native(ctx):
    """the same statement built by the library (og_deposit_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_deposit_r1cs(ctx._h, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_deposit_inputs(nullifier, secret, depositor):
    """one deposit record: 3 x 32 B, nullifier | secret | depositor (include/owshen_gpu.h)"""
    return _pack((nullifier, secret, depositor))


def deposit_witness(ctx, inputs_d):
    """inputs_d: device uint8 [n, 3, 32] -> device uint8 [n, 735, 32] (og_deposit_witness_d)"""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (D_N_REC, 32)
    shp = (C.c_uint64 * 3)()
    ctx._check(ctx._lib.og_deposit_shape(shp))
    assert (int(shp[0]), int(shp[1]), int(shp[2])) == (*deposit_shape(), D_N_PUB), "circuit.py and witness.hip disagree on the deposit shape"
    out = ctx.empty(n, int(shp[0]), 32)
    ctx._pre()
    ctx._check(ctx._lib.og_deposit_witness_d(ctx._h, ctx.ptr(inputs_d), n, ctx.ptr(out)))
    return out


def deposit_prove(ctx, pk, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 3, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_deposit_prove_batch_d);
    return_public: also (commitment, depositor) of every proof, np.uint8 [n, 2, 32]"""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (D_N_REC, 32)
    rsb = pk._rs_bytes(rs)
    assert rsb.shape[0] == n
    out = np.zeros((n, 256), dtype=np.uint8)
    pub = np.zeros((n, D_N_PUB, 32), dtype=np.uint8) if return_public else None
    ctx._pre()
    ctx._check(ctx._lib.og_deposit_prove_batch_d(ctx._h, pk._h, ctx.ptr(inputs_d), n, rsb.ctypes.data_as(C.c_void_p),
                                                 out.ctypes.data_as(C.c_void_p), pub.ctypes.data_as(C.c_void_p) if return_public else None))
    return (out, pub) if return_public else out


# ---- the split statement (tests/split_spec.py is the spec; witness.hip k_split_core fills the wires) --------------------------------
# public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf; private: nullifier, secret, amount,
# change_commitment, change, the path.  leaf = H(H(nullifier, secret), H(amount, token)) under root; amount_out + change = amount,
# both below 2^128 by a bit decomposition; change_leaf = H(change_commitment, H(change, token)).  The reference's withdraw
# (/root/reference/src/services/api_services/withdraw.rs:27-71) burns a whole amount; with this statement part of a note leaves
# the pool and the rest stays in it as a fresh note.
S_N_PUB, S_N_REC, S_N_BITS = 7, 9, 128
(SW_ROOT, SW_NH, SW_RECIPIENT, SW_AMOUNT_OUT, SW_TOKEN, SW_CHAIN, SW_CHANGE_LEAF, SW_NULLIFIER, SW_SECRET, SW_AMOUNT, SW_CHANGE_COMMITMENT,
 SW_CHANGE) = range(1, 13)


def split_shape(depth):
    """(n_wires, n_constraints): (28104, 28065) at depth 32"""
    return 1 + S_N_PUB + 5 + 2 * depth + 2 + 2 * S_N_BITS + depth + (6 + depth) * 730 - 3, 3 + 2 * (S_N_BITS + 1) + 2 * depth + (6 + depth) * 730


def split_r1cs(mimc7_constants, depth=32):
    """the split statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = split_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + S_N_PUB + 5)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_rsq = bld.alloc()
    w_csq = bld.alloc()
    w_obit = bld.alloc(S_N_BITS)
    w_cbit = bld.alloc(S_N_BITS)
    bld.enforce([(SW_RECIPIENT, 1)], [(SW_RECIPIENT, 1)], [(w_rsq, 1)])
    bld.enforce([(SW_CHAIN, 1)], [(SW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(SW_AMOUNT_OUT, 1), (SW_CHANGE, 1)], [(0, 1)], [(SW_AMOUNT, 1)])
    bld.range_check(SW_AMOUNT_OUT, w_obit, S_N_BITS)
    bld.range_check(SW_CHANGE, w_cbit, S_N_BITS)
    bld.spend_note(SW_NULLIFIER, SW_SECRET, SW_AMOUNT, SW_TOKEN, SW_NH, w_sib, w_bit, depth, SW_ROOT)
    change_asset = bld.hash2([(SW_CHANGE, 1)], [(SW_TOKEN, 1)])
    bld.hash2([(SW_CHANGE_COMMITMENT, 1)], [(change_asset, 1)], out_wire=SW_CHANGE_LEAF)
    return _finish(bld, n_wires, S_N_PUB, n_constraints)


def split_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_split_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_split_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_split_inputs(nullifier, secret, amount, recipient, amount_out, index, siblings, token=0, chain_id=0, change_commitment=0):
    """one split record: (9 + depth) x 32 B (include/owshen_gpu.h):
    nullifier | secret | amount | recipient | amount_out | index | token | chain_id | change_commitment | siblings[depth]"""
    return _pack([nullifier, secret, amount, recipient, amount_out, index, token, chain_id, change_commitment] + list(siblings))


def split_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 9 + depth, 32] -> device uint8 [n, n_wires, 32] (og_split_witness_d)"""
    return _records_witness(ctx, "split", S_N_REC + depth, depth, inputs_d, split_shape(depth), S_N_PUB)


def split_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 9 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_split_prove_batch_d);
    return_public: also (root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf) of every proof, np.uint8 [n, 7, 32]"""
    return _records_prove(ctx, pk, "split", S_N_REC + depth, S_N_PUB, depth, inputs_d, rs, return_public)


def split_change_leaf(change_commitment, change, token, ctx):
    """the ledger's side of a split: the leaf of the change note, H(change_commitment, H(change, token)), through og_mimc7_hash2_d
    (the value of public input 7; what og_mimc7_append_d appends).  Returns an int."""
    leaf = ctx.mimc7_hash2(_dev(ctx, change_commitment), ctx.mimc7_hash2(_dev(ctx, change), _dev(ctx, token)))
    return int.from_bytes(ctx.to_host(leaf).tobytes(), "little")


# ---- the join statement (tests/join_spec.py is the spec; witness.hip k_join_core fills the wires) -----------------------------------
# public: root, nullifier_hash_a, nullifier_hash_b, chain_id, out_leaf; private: per note nullifier, secret, amount and a path; token,
# out_commitment, sum, nh_diff_inv.  Both notes lie under root (both walks end in wire 1), amount_a + amount_b = sum with all three
# below 2^128 by a bit decomposition, (nullifier_hash_a - nullifier_hash_b) nh_diff_inv = 1, out_leaf = H(out_commitment,
# H(sum, token)).  The inverse of split: two notes are spent, one note worth their sum is created, nothing leaves the pool.
J_N_PUB, J_N_REC, J_N_BITS = 5, 11, 128
JW_ROOT, JW_NH_A, JW_NH_B, JW_CHAIN, JW_OUT_LEAF = range(1, 6)
JW_NOTE_A, JW_NOTE_B = 6, 9                    # a note: nullifier, secret, amount
JW_TOKEN, JW_OUT_COMMITMENT, JW_SUM, JW_NH_DIFF_INV = range(12, 16)


def join_shape(depth):
    """(n_wires, n_constraints): (54608, 54538) at depth 32"""
    return 396 + 6 * depth + (10 + 2 * depth) * 730, 390 + 4 * depth + (10 + 2 * depth) * 730


def join_r1cs(mimc7_constants, depth=32):
    """the join statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = join_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + J_N_PUB + 10)
    w_sib = bld.alloc(2 * depth)
    w_bit = bld.alloc(2 * depth)
    w_csq = bld.alloc()
    w_bits = bld.alloc(3 * J_N_BITS)
    bld.enforce([(JW_CHAIN, 1)], [(JW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(JW_NOTE_A + 2, 1), (JW_NOTE_B + 2, 1)], [(0, 1)], [(JW_SUM, 1)])
    bld.enforce([(JW_NH_A, 1), (JW_NH_B, R - 1)], [(JW_NH_DIFF_INV, 1)], [(0, 1)])      # two different notes
    for v, value in enumerate((JW_NOTE_A + 2, JW_NOTE_B + 2, JW_SUM)):
        bld.range_check(value, w_bits + v * J_N_BITS, J_N_BITS)
    for x, (note, w_nh) in enumerate(((JW_NOTE_A, JW_NH_A), (JW_NOTE_B, JW_NH_B))):   # both walks end in wire 1
        bld.spend_note(note, note + 1, note + 2, JW_TOKEN, w_nh, w_sib + x * depth, w_bit + x * depth, depth, JW_ROOT)
    out_asset = bld.hash2([(JW_SUM, 1)], [(JW_TOKEN, 1)])
    bld.hash2([(JW_OUT_COMMITMENT, 1)], [(out_asset, 1)], out_wire=JW_OUT_LEAF)
    return _finish(bld, n_wires, J_N_PUB, n_constraints)


def join_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_join_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_join_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_join_inputs(nullifier_a, secret_a, amount_a, index_a, siblings_a, nullifier_b, secret_b, amount_b, index_b, siblings_b, token=0,
                     chain_id=0, out_commitment=0):
    """one join record: (11 + 2 depth) x 32 B (include/owshen_gpu.h):
    nullifier_a | secret_a | amount_a | index_a | nullifier_b | secret_b | amount_b | index_b | token | chain_id | out_commitment
    | siblings_a[depth] | siblings_b[depth]"""
    assert len(siblings_a) == len(siblings_b)
    vals = [nullifier_a, secret_a, amount_a, index_a, nullifier_b, secret_b, amount_b, index_b, token, chain_id, out_commitment]
    return _pack(vals + list(siblings_a) + list(siblings_b))


def join_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 11 + 2 depth, 32] -> device uint8 [n, n_wires, 32] (og_join_witness_d)"""
    return _records_witness(ctx, "join", J_N_REC + 2 * depth, depth, inputs_d, join_shape(depth), J_N_PUB)


def join_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 11 + 2 depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_join_prove_batch_d);
    return_public: also (root, nullifier_hash_a, nullifier_hash_b, chain_id, out_leaf) of every proof, np.uint8 [n, 5, 32]"""
    return _records_prove(ctx, pk, "join", J_N_REC + 2 * depth, J_N_PUB, depth, inputs_d, rs, return_public)


def join_out_leaf(out_commitment, total, token, ctx):
    """the ledger's and the receiver's side of a join: the leaf of the joined note, H(out_commitment, H(sum, token)), through
    og_mimc7_hash2_d (the value of public input 5; what og_mimc7_append_d appends).  Returns an int."""
    leaf = ctx.mimc7_hash2(_dev(ctx, out_commitment), ctx.mimc7_hash2(_dev(ctx, total), _dev(ctx, token)))
    return int.from_bytes(ctx.to_host(leaf).tobytes(), "little")


# ---- the transfer statement (tests/transfer_spec.py is the spec; witness.hip k_transfer_core / k_tw9_* fill the wires) ---------------
# public: root, nullifier_hash, chain_id, pay_leaf, change_leaf; private: nullifier, secret, amount, token, pay_commitment, pay_amount,
# change_commitment, change, the path.  leaf = H(H(nullifier, secret), H(amount, token)) under root; pay_amount + change = amount, both
# below 2^128 by a bit decomposition; pay_leaf = H(pay_commitment, H(pay_amount, token)), change_leaf = H(change_commitment,
# H(change, token)).  One note is spent, two are created -- one for the payee, one for the payer -- and nothing leaves the pool.
T_N_PUB, T_N_REC, T_N_BITS = 5, 9, 128
(TW_ROOT, TW_NH, TW_CHAIN, TW_PAY_LEAF, TW_CHANGE_LEAF, TW_NULLIFIER, TW_SECRET, TW_AMOUNT, TW_TOKEN, TW_PAY_COMMITMENT, TW_PAY_AMOUNT,
 TW_CHANGE_COMMITMENT, TW_CHANGE) = range(1, 14)


def transfer_shape(depth):
    """(n_wires, n_constraints): (29563, 29524) at depth 32"""
    return 267 + 3 * depth + (8 + depth) * 730, 260 + 2 * depth + (8 + depth) * 730


def transfer_r1cs(mimc7_constants, depth=32):
    """the transfer statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = transfer_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + T_N_PUB + 8)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_csq = bld.alloc()
    w_pbit = bld.alloc(T_N_BITS)
    w_cbit = bld.alloc(T_N_BITS)
    bld.enforce([(TW_CHAIN, 1)], [(TW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(TW_PAY_AMOUNT, 1), (TW_CHANGE, 1)], [(0, 1)], [(TW_AMOUNT, 1)])
    bld.range_check(TW_PAY_AMOUNT, w_pbit, T_N_BITS)
    bld.range_check(TW_CHANGE, w_cbit, T_N_BITS)
    bld.spend_note(TW_NULLIFIER, TW_SECRET, TW_AMOUNT, TW_TOKEN, TW_NH, w_sib, w_bit, depth, TW_ROOT)
    pay_asset = bld.hash2([(TW_PAY_AMOUNT, 1)], [(TW_TOKEN, 1)])
    bld.hash2([(TW_PAY_COMMITMENT, 1)], [(pay_asset, 1)], out_wire=TW_PAY_LEAF)
    change_asset = bld.hash2([(TW_CHANGE, 1)], [(TW_TOKEN, 1)])
    bld.hash2([(TW_CHANGE_COMMITMENT, 1)], [(change_asset, 1)], out_wire=TW_CHANGE_LEAF)
    return _finish(bld, n_wires, T_N_PUB, n_constraints)


def transfer_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_transfer_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_transfer_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_transfer_inputs(nullifier, secret, amount, index, siblings, token=0, chain_id=0, pay_commitment=0, pay_amount=0, change_commitment=0):
    """one transfer record: (9 + depth) x 32 B (include/owshen_gpu.h):
    nullifier | secret | amount | index | token | chain_id | pay_commitment | pay_amount | change_commitment | siblings[depth]"""
    return _pack([nullifier, secret, amount, index, token, chain_id, pay_commitment, pay_amount, change_commitment] + list(siblings))


def transfer_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 9 + depth, 32] -> device uint8 [n, n_wires, 32] (og_transfer_witness_d)"""
    return _records_witness(ctx, "transfer", T_N_REC + depth, depth, inputs_d, transfer_shape(depth), T_N_PUB)


def transfer_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 9 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_transfer_prove_batch_d);
    return_public: also (root, nullifier_hash, chain_id, pay_leaf, change_leaf) of every proof, np.uint8 [n, 5, 32]"""
    return _records_prove(ctx, pk, "transfer", T_N_REC + depth, T_N_PUB, depth, inputs_d, rs, return_public)


def transfer_leaves(pay_commitment, pay_amount, change_commitment, change, token, ctx):
    """the ledger's and the payee's side of a transfer: (pay_leaf, change_leaf) = (H(pay_commitment, H(pay_amount, token)),
    H(change_commitment, H(change, token))) through og_mimc7_hash2_d -- the values of public inputs 4 and 5, what og_mimc7_append_d
    appends, in this order.  Returns two ints."""
    tok = _dev(ctx, token, token)
    leaves = ctx.mimc7_hash2(_dev(ctx, pay_commitment, change_commitment), ctx.mimc7_hash2(_dev(ctx, pay_amount, change), tok))
    return tuple(int.from_bytes(row.tobytes(), "little") for row in ctx.to_host(leaves))


# ---- the claim statement (tests/claim_spec.py is the spec; witness.hip k_claim_core fills the wires) -----------------------------------
# public: root, nullifier_hash, chain_id, out_leaf; private: x, amount, token, out_commitment, the path.  An owned note
# (og_note_seal_owned_batch_d) is bound to a one-time key P = pk + t BASE; only the payee knows x = sk + t mod l with P = x BASE.
# x = sum 2^i b_i over 251 boolean wires with x < l; c = H(P.x, P.y); leaf = H(c, asset = H(amount, token)) under root;
# nullifier_hash = H(x, 1); out_leaf = H(out_commitment, asset) -- an ordinary note of the same value that only the claimant opens.
C_N_PUB, C_N_REC, C_N_BITS = 4, 6, 251
C_N_CMP = bin(ED_L - 1).count("1")     # 114: the comparison's wires
(CW_ROOT, CW_NH, CW_CHAIN, CW_OUT_LEAF, CW_X, CW_AMOUNT, CW_TOKEN, CW_OUT_COMMITMENT) = range(1, 9)


def claim_shape(depth):
    """(n_wires, n_constraints): (28733, 28834) at depth 32"""
    return 1627 + 3 * depth + (5 + depth) * 730, 3 + 6 * C_N_BITS + C_N_BITS + 730 * (5 + depth) + 2 * depth


def claim_r1cs(mimc7_constants, depth=32):
    """the claim statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = claim_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + C_N_PUB + 4)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_csq = bld.alloc()
    w_xbit = bld.alloc(C_N_BITS)
    bld.enforce([(CW_CHAIN, 1)], [(CW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(w_xbit + i, 1 << i) for i in range(C_N_BITS)], [(0, 1)], [(CW_X, 1)])
    bld.enforce([(0, 1)], [(0, 1)], [(0, 1)])
    bld.less_equal_const(w_xbit, C_N_BITS, ED_L - 1)
    px, py = bld.fixed_base_mul(w_xbit, C_N_BITS)
    c = bld.hash2(px, py)
    asset = bld.hash2([(CW_AMOUNT, 1)], [(CW_TOKEN, 1)])
    leaf = bld.hash2([(c, 1)], [(asset, 1)])
    bld.hash2([(CW_X, 1)], [(0, 1)], out_wire=CW_NH)
    bld.merkle_walk(leaf, w_sib, w_bit, depth, CW_ROOT)
    bld.hash2([(CW_OUT_COMMITMENT, 1)], [(asset, 1)], out_wire=CW_OUT_LEAF)
    return _finish(bld, n_wires, C_N_PUB, n_constraints)


def claim_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_claim_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_claim_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_claim_inputs(x, amount, index, siblings, token=0, chain_id=0, out_commitment=0):
    """one claim record: (6 + depth) x 32 B (include/owshen_gpu.h):
    x | amount | token | chain_id | out_commitment | index | siblings[depth]"""
    return _pack([x, amount, token, chain_id, out_commitment, index] + list(siblings))


def claim_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 6 + depth, 32] -> device uint8 [n, n_wires, 32] (og_claim_witness_d)"""
    return _records_witness(ctx, "claim", C_N_REC + depth, depth, inputs_d, claim_shape(depth), C_N_PUB)


def claim_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 6 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_claim_prove_batch_d);
    return_public: also (root, nullifier_hash, chain_id, out_leaf) of every proof, np.uint8 [n, 4, 32]"""
    return _records_prove(ctx, pk, "claim", C_N_REC + depth, C_N_PUB, depth, inputs_d, rs, return_public)


def claim_out_leaf(out_commitment, amount, token, ctx):
    """the ledger's and the claimant's side of a claim: out_leaf = H(out_commitment, H(amount, token)) through og_mimc7_hash2_d (the
    value of public input 4; what og_mimc7_append_d appends).  Returns an int."""
    leaf = ctx.mimc7_hash2(_dev(ctx, out_commitment), ctx.mimc7_hash2(_dev(ctx, amount), _dev(ctx, token)))
    return int.from_bytes(ctx.to_host(leaf).tobytes(), "little")


# ---- the send and the redeem statement (tests/send_spec.py, tests/redeem_spec.py are the specs; witness.hip k_send_core and
# k_redeem_core fill the wires): claim's front -- the bits of x, x < l, P = x BASE, c = H(P), leaf = H(c, H(amount, token)) under root,
# nullifier_hash = H(x, 1), the SAME hash for all three owned statements -- in front of transfer's and of split's back.  An owned note
# is spent directly: no claim first.
def _owned_front(bld, w_x, w_amount, w_token, w_nh, w_xbit, w_sib, w_bit, depth, w_root):
    """the rows all owned statements share behind their own first rows: the recomposition of x, the comparison, the multiplication,
    then the gadgets c, asset, leaf, nullifier_hash and the path (claim keeps its own text: a one * one row follows its recomposition)"""
    bld.enforce([(w_xbit + i, 1 << i) for i in range(C_N_BITS)], [(0, 1)], [(w_x, 1)])
    bld.less_equal_const(w_xbit, C_N_BITS, ED_L - 1)
    px, py = bld.fixed_base_mul(w_xbit, C_N_BITS)
    c = bld.hash2(px, py)
    asset = bld.hash2([(w_amount, 1)], [(w_token, 1)])
    leaf = bld.hash2([(c, 1)], [(asset, 1)])
    bld.hash2([(w_x, 1)], [(0, 1)], out_wire=w_nh)
    bld.merkle_walk(leaf, w_sib, w_bit, depth, w_root)


# send -- public: root, nullifier_hash, chain_id, pay_leaf, change_leaf (transfer's list); private: x, amount, token, pay_commitment,
# pay_amount, change_commitment, change, the path
SN_N_PUB, SN_N_REC, SN_N_BITS = 5, 8, 128
(SNW_ROOT, SNW_NH, SNW_CHAIN, SNW_PAY_LEAF, SNW_CHANGE_LEAF, SNW_X, SNW_AMOUNT, SNW_TOKEN, SNW_PAY_COMMITMENT, SNW_PAY_AMOUNT, SNW_CHANGE_COMMITMENT,
 SNW_CHANGE) = range(1, 13)


def send_shape(depth):
    """(n_wires, n_constraints): (31182, 31282) at depth 32"""
    return 1886 + 3 * depth + (8 + depth) * 730, 2018 + 2 * depth + (8 + depth) * 730


def send_r1cs(mimc7_constants, depth=32):
    """the send statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = send_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + SN_N_PUB + 7)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_csq = bld.alloc()
    w_pbit = bld.alloc(SN_N_BITS)
    w_cbit = bld.alloc(SN_N_BITS)
    w_xbit = bld.alloc(C_N_BITS)
    bld.enforce([(SNW_CHAIN, 1)], [(SNW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(SNW_PAY_AMOUNT, 1), (SNW_CHANGE, 1)], [(0, 1)], [(SNW_AMOUNT, 1)])
    bld.range_check(SNW_PAY_AMOUNT, w_pbit, SN_N_BITS)
    bld.range_check(SNW_CHANGE, w_cbit, SN_N_BITS)
    _owned_front(bld, SNW_X, SNW_AMOUNT, SNW_TOKEN, SNW_NH, w_xbit, w_sib, w_bit, depth, SNW_ROOT)
    pay_asset = bld.hash2([(SNW_PAY_AMOUNT, 1)], [(SNW_TOKEN, 1)])
    bld.hash2([(SNW_PAY_COMMITMENT, 1)], [(pay_asset, 1)], out_wire=SNW_PAY_LEAF)
    change_asset = bld.hash2([(SNW_CHANGE, 1)], [(SNW_TOKEN, 1)])
    bld.hash2([(SNW_CHANGE_COMMITMENT, 1)], [(change_asset, 1)], out_wire=SNW_CHANGE_LEAF)
    return _finish(bld, n_wires, SN_N_PUB, n_constraints)


def send_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_send_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_send_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_send_inputs(x, amount, index, siblings, token=0, chain_id=0, pay_commitment=0, pay_amount=0, change_commitment=0):
    """one send record: (8 + depth) x 32 B (include/owshen_gpu.h):
    x | amount | token | chain_id | pay_commitment | pay_amount | change_commitment | index | siblings[depth]"""
    return _pack([x, amount, token, chain_id, pay_commitment, pay_amount, change_commitment, index] + list(siblings))


def send_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 8 + depth, 32] -> device uint8 [n, n_wires, 32] (og_send_witness_d)"""
    return _records_witness(ctx, "send", SN_N_REC + depth, depth, inputs_d, send_shape(depth), SN_N_PUB)


def send_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 8 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_send_prove_batch_d);
    return_public: also (root, nullifier_hash, chain_id, pay_leaf, change_leaf) of every proof, np.uint8 [n, 5, 32]"""
    return _records_prove(ctx, pk, "send", SN_N_REC + depth, SN_N_PUB, depth, inputs_d, rs, return_public)


def send_leaves(pay_commitment, pay_amount, change_commitment, change, token, ctx):
    """the ledger's and the payee's side of a send: (pay_leaf, change_leaf), the values of public inputs 4 and 5, what
    og_mimc7_append_d appends, in this order -- the two leaves of a transfer.  Returns two ints."""
    return transfer_leaves(pay_commitment, pay_amount, change_commitment, change, token, ctx)


# redeem -- public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf (split's list); private: x, amount,
# change_commitment, change, the path
RD_N_PUB, RD_N_REC, RD_N_BITS = 7, 8, 128
(RDW_ROOT, RDW_NH, RDW_RECIPIENT, RDW_AMOUNT_OUT, RDW_TOKEN, RDW_CHAIN, RDW_CHANGE_LEAF, RDW_X, RDW_AMOUNT, RDW_CHANGE_COMMITMENT, RDW_CHANGE) = range(1, 12)


def redeem_shape(depth):
    """(n_wires, n_constraints): (29723, 29823) at depth 32"""
    return 1887 + 3 * depth + (6 + depth) * 730, 2019 + 2 * depth + (6 + depth) * 730


def redeem_r1cs(mimc7_constants, depth=32):
    """the redeem statement as an R1CS (the same gadget builder as the withdraw circuit); no padding gates"""
    assert depth >= 1 and len(mimc7_constants) == N_ROUNDS
    n_wires, n_constraints = redeem_shape(depth)
    bld = _Builder([int(c) for c in mimc7_constants])
    bld.alloc(1 + RD_N_PUB + 4)
    w_sib = bld.alloc(depth)
    w_bit = bld.alloc(depth)
    w_rsq = bld.alloc()
    w_csq = bld.alloc()
    w_obit = bld.alloc(RD_N_BITS)
    w_cbit = bld.alloc(RD_N_BITS)
    w_xbit = bld.alloc(C_N_BITS)
    bld.enforce([(RDW_RECIPIENT, 1)], [(RDW_RECIPIENT, 1)], [(w_rsq, 1)])
    bld.enforce([(RDW_CHAIN, 1)], [(RDW_CHAIN, 1)], [(w_csq, 1)])
    bld.enforce([(RDW_AMOUNT_OUT, 1), (RDW_CHANGE, 1)], [(0, 1)], [(RDW_AMOUNT, 1)])
    bld.range_check(RDW_AMOUNT_OUT, w_obit, RD_N_BITS)
    bld.range_check(RDW_CHANGE, w_cbit, RD_N_BITS)
    _owned_front(bld, RDW_X, RDW_AMOUNT, RDW_TOKEN, RDW_NH, w_xbit, w_sib, w_bit, depth, RDW_ROOT)
    change_asset = bld.hash2([(RDW_CHANGE, 1)], [(RDW_TOKEN, 1)])
    bld.hash2([(RDW_CHANGE_COMMITMENT, 1)], [(change_asset, 1)], out_wire=RDW_CHANGE_LEAF)
    return _finish(bld, n_wires, RD_N_PUB, n_constraints)


def redeem_r1cs_native(ctx, depth=32):
    """the same statement built by the library (og_redeem_r1cs: what a Rust host calls)"""
    h = C.c_void_p()
    ctx._check(ctx._lib.og_redeem_r1cs(ctx._h, depth, C.byref(h)))
    return _r1cs_from_handle(ctx, h)


def pack_redeem_inputs(x, amount, recipient, amount_out, index, siblings, token=0, chain_id=0, change_commitment=0):
    """one redeem record: (8 + depth) x 32 B (include/owshen_gpu.h):
    x | amount | recipient | amount_out | token | chain_id | change_commitment | index | siblings[depth]"""
    return _pack([x, amount, recipient, amount_out, token, chain_id, change_commitment, index] + list(siblings))


def redeem_witness(ctx, depth, inputs_d):
    """inputs_d: device uint8 [n, 8 + depth, 32] -> device uint8 [n, n_wires, 32] (og_redeem_witness_d)"""
    return _records_witness(ctx, "redeem", RD_N_REC + depth, depth, inputs_d, redeem_shape(depth), RD_N_PUB)


def redeem_prove(ctx, pk, depth, inputs_d, rs, return_public=False):
    """inputs_d: device uint8 [n, 8 + depth, 32]; rs: (r, s) pairs or uint8 [n, 64] -> np.uint8 [n, 256] (og_redeem_prove_batch_d);
    return_public: also (root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf) of every proof, np.uint8 [n, 7, 32]"""
    return _records_prove(ctx, pk, "redeem", RD_N_REC + depth, RD_N_PUB, depth, inputs_d, rs, return_public)


def redeem_change_leaf(change_commitment, change, token, ctx):
    """the ledger's side of a redeem: the leaf of the change note, H(change_commitment, H(change, token)) (the value of public input
    7; what og_mimc7_append_d appends).  Returns an int."""
    return split_change_leaf(change_commitment, change, token, ctx)


class ProveJob:
    """One submitted batch (og_withdraw_prove_batch_submit_d): keeps the host buffers the library fills alive until `wait`."""

    def __init__(self, ctx, handle, out, pub, rsb, inputs_d):
        self._ctx, self._h, self._out, self._pub, self._keep = ctx, handle, out, pub, (rsb, inputs_d)

    def wait(self):
        """blocks until the batch is proved; returns proofs np.uint8 [n, 256] (and the public inputs [n, 6, 32] when asked for)"""
        if self._h is not None:
            h, self._h = self._h, None
            self._ctx._check(self._ctx._lib.og_job_wait(self._ctx._h, h))
        return (self._out, self._pub) if self._pub is not None else self._out

    def done(self):
        """non-blocking (og_job_poll): True once every kernel of the batch has finished, i.e. `wait` would return at once"""
        if self._h is None:
            return True
        flag = C.c_int(0)
        self._ctx._check(self._ctx._lib.og_job_poll(self._ctx._h, self._h, C.byref(flag)))
        return bool(flag.value)

    def abandon(self):
        """the results are no longer wanted (og_job_abandon): waits for the job's kernels, copies nothing out, frees the call slot"""
        if self._h is not None:
            h, self._h = self._h, None
            self._ctx._check(self._ctx._lib.og_job_abandon(self._ctx._h, h))

    def __del__(self):
        # a job dropped without wait() must not keep its call slot, nor leave the library writing into freed host buffers
        try:
            if self._h is not None and self._ctx._h:
                self.abandon()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def submit_from_inputs(ctx, pk, depth, inputs_d, rs, n_pad3=0, n_pad2=0, return_public=False):
    """prove_from_inputs in two halves: enqueue the whole batch and return a ProveJob; `job.wait()` delivers the proofs.  Submit
    the next batch before waiting for the current one and its cold start runs under the current batch's last accumulations
    (at most two batches in flight per context)."""
    n = inputs_d.shape[0]
    assert tuple(inputs_d.shape[1:]) == (N_REC + depth, 32)
    rsb = pk._rs_bytes(rs)
    assert rsb.shape[0] == n
    out = np.zeros((n, 256), dtype=np.uint8)
    pub = np.zeros((n, N_PUB, 32), dtype=np.uint8) if return_public else None
    ctx._pre()
    h = C.c_void_p()
    ctx._check(ctx._lib.og_withdraw_prove_batch_submit_d(ctx._h, pk._h, depth, n_pad3, n_pad2, ctx.ptr(inputs_d), n,
                                                         rsb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                         pub.ctypes.data_as(C.c_void_p) if return_public else None, C.byref(h)))
    return ProveJob(ctx, h, out, pub, rsb, inputs_d)
