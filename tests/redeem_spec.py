"""The redeem statement -- specification + witness generator.  TEST INFRASTRUCTURE ONLY.

No reference counterpart: the snapshot contains no circuit.  This file DEFINES the eighth statement of the pool: the
front of tests/claim_spec.py (whose gadgets `compare` and `fixed_base` it reuses) with the back of tests/split_spec.py.  The product's
builders (owshen_amd/circuit.py redeem_r1cs, og_redeem_r1cs in keygen.hip) and the HIP witness kernel (witness.hip k_redeem_core) are
checked against it.

Statement (public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf; n_pub = 7 -- split's list):
    "I know the discrete logarithm x of the one-time key P of an owned note (tests/owned_note_spec.py) under `root`.  It is spent.  I
     take `amount_out` of it out to `recipient`, and the rest goes into the new leaf `change_leaf`."  It is `split` for an owned note:
     the payee needs no `claim` in front of it.
Private: x, amount, change_commitment, change, the path.  `amount` stays private.  With H = MultiMiMC7 2-to-1:
    x = sum 2^i b_i over 251 boolean wires, and x < l;
    P = x BASE, c = H(P.x, P.y), asset = H(amount, token);
    leaf = H(c, asset) is under `root` at `index`;
    nullifier_hash = H(x, 1) -- what `claim` and `send` publish for the same note: one spent set;
    amount_out + change = amount, with amount_out < 2^128 and change < 2^128, each by a 128-bit decomposition;
    change_leaf = H(change_commitment, H(change, token)), over the ONE token wire;
    `recipient` and `chain_id` are bound by a square each.
`change_commitment` is unconstrained: an ordinary c' or the c of an owned or view note.  There is no one * one = one row.

The ledger's part of a redeem, in order: verify the proof; check that `root` is known; check that `nullifier_hash` is unspent, and
mark it; pay `amount_out` of `token` to `recipient`; append `change_leaf` (og_mimc7_append_d).

Wire order (the contract all implementations share):
    0 one | 1 root | 2 nullifier_hash | 3 recipient | 4 amount_out | 5 token | 6 chain_id | 7 change_leaf
    8 x | 9 amount | 10 change_commitment | 11 change
    12.. siblings[D] | index bits[D] | recipient^2 | chain_id^2 | amount_out bits[128] (LSB first) | change bits[128]
       | x bits[251] (LSB first) | the comparison's t wires[114] | the multiplication's wires[5 x 251]
    gadgets in the order: c, asset, leaf, nullifier_hash (out = wire 2), level 0..D-1 (each first allocates left_l; the last one's
      out = wire 1), change_asset, change_leaf (out = wire 7)
Constraint order: recipient^2; chain_id^2; (amount_out + change) * 1 = amount; the 129 range rows of amount_out; the 129 range rows of
change; (sum 2^i b_i) * 1 = x; the comparison's 251 rows, bit 250 first; the multiplication's 1506 rows, bit 0 first; the gadgets in
the order above, with levels as in `claim`.
"""
from oracle.py.fields import R
from oracle.py import babyjubjub as bj
from oracle.py import mimc7
from oracle.py.withdraw import _CS, _hash2, _lc_add
from tests.claim_spec import ELL, M, N_CMP, compare, fixed_base, nullifier_hash_of
from tests.transfer_spec import _ForgedCS, _range

N_PUB = 7
N_BITS = 251        # of x
N_RANGE = 128       # of an amount
ROW_SUM = 2
ROW_OUT_RANGE = 3 + N_RANGE          # 131: the recomposition of amount_out
ROW_CHANGE_RANGE = 4 + 2 * N_RANGE   # 260: the recomposition of change
ROW_RECOMPOSE = ROW_CHANGE_RANGE + 1  # 261: the recomposition of x
ROW_CMP = ROW_RECOMPOSE + 1          # 262: the comparison's first row (bit 250)
ROW_MUL = ROW_CMP + N_BITS           # 513: the multiplication's first row (bit 0's booleanity)
ROW_GADGETS = ROW_MUL + 6 * N_BITS   # 2019


def shape(depth):
    """(n_wires, n_constraints): (7000, 7131) at depth 1, (7733, 7863) at 2, (29723, 29823) at 32"""
    return 1887 + 3 * depth + (6 + depth) * 730, 2019 + 2 * depth + (6 + depth) * 730


def gadget_row(depth, h):
    """the first row of gadget h (0 c, 1 asset, 2 leaf, 3 nullifier_hash, 4 + l level l -- its booleanity row --, 4 + D change_asset,
    5 + D change_leaf); a gadget's hash is 730 rows and its output row is the last of them"""
    return ROW_GADGETS + 730 * h + 2 * min(max(h - 4, 0), depth)


def first_range_wire(depth):
    return 14 + 2 * depth


def first_bit_wire(depth):
    """the first bit wire of x"""
    return 270 + 2 * depth


def change_leaf_of(change_commitment, change, token):
    return mimc7.hash2(change_commitment, mimc7.hash2(change, token))


def build(depth, x, amount, recipient, amount_out, index, siblings, token=0, chain_id=0, change_commitment=0, forge=None):
    """returns (n_wires, n_pub, constraints, witness z).
    forge = {"bits": [251 values], "x": v, "change": v, "change_leaf": v, "change_asset_token": v} (any may be missing) assembles a
    witness that is wrong on purpose: the bit wires of x are forge["bits"], the wire x and the nullifier hash are those of forge["x"]
    (every wire of the comparison and of the multiplication follows from the forged bits as an honest prover's would); the amounts are
    taken as given (as field elements, `change` = amount - amount_out mod r unless forged; the range bit wires are the low 128 bits);
    wire 7 is forge["change_leaf"]; the wires of the change_asset gadget are those of H(change, forge["change_asset_token"]).  No row
    is checked here: the caller finds the rows that fail."""
    assert len(siblings) == depth >= 1
    forge_of = forge or {}
    if forge is None:
        assert 0 <= x < ELL and 0 <= amount_out <= amount < (1 << N_RANGE)
    change = forge_of.get("change", (amount - amount_out) % R)
    cs = _CS() if forge is None else _ForgedCS()
    bits = forge_of.get("bits", [(x >> i) & 1 for i in range(N_BITS)])
    assert len(bits) == N_BITS
    xw = forge_of.get("x", x)
    change_token = forge_of.get("change_asset_token", token)
    change_leaf = change_leaf_of(change_commitment, change, change_token)
    w_root, w_nh, w_rcp, w_out = cs.alloc(0), cs.alloc(nullifier_hash_of(xw)), cs.alloc(recipient), cs.alloc(amount_out)
    w_tok, w_chain, w_cleaf = cs.alloc(token), cs.alloc(chain_id), cs.alloc(forge_of.get("change_leaf", change_leaf))
    w_x, w_amt, w_cc, w_chg = cs.alloc(xw), cs.alloc(amount), cs.alloc(change_commitment), cs.alloc(change)
    w_sib = [cs.alloc(s) for s in siblings]
    w_bit = [cs.alloc((index >> l) & 1) for l in range(depth)]
    w_rsq = cs.alloc(recipient * recipient)
    w_csq = cs.alloc(chain_id * chain_id)
    w_obit = [cs.alloc((amount_out >> i) & 1) for i in range(N_RANGE)]
    w_cbit = [cs.alloc((change >> i) & 1) for i in range(N_RANGE)]
    w_xbit = [cs.alloc(b) for b in bits]
    assert w_obit[0] == first_range_wire(depth) and w_xbit[0] == first_bit_wire(depth)
    # the root an honest prover's wire 1 holds, before the rows that bind it are written
    cs2 = _ForgedCS()
    cs2.z = list(cs.z)
    px, py = fixed_base(cs2, w_xbit)
    c_val = mimc7.hash2(cs2.val(px), cs2.val(py))
    cs.z[w_root] = mimc7.merkle_root_from_path(mimc7.hash2(c_val, mimc7.hash2(amount, token)), index, siblings)[-1]
    cs.enforce({w_rcp: 1}, {w_rcp: 1}, {w_rsq: 1})
    cs.enforce({w_chain: 1}, {w_chain: 1}, {w_csq: 1})
    cs.enforce({w_out: 1, w_chg: 1}, {0: 1}, {w_amt: 1})
    _range(cs, w_out, w_obit)
    assert len(cs.constraints) == ROW_OUT_RANGE + 1
    _range(cs, w_chg, w_cbit)
    assert len(cs.constraints) == ROW_RECOMPOSE
    cs.enforce({b: 1 << i for i, b in enumerate(w_xbit)}, {0: 1}, {w_x: 1})
    assert len(cs.constraints) == ROW_CMP
    compare(cs, w_xbit, M)
    assert len(cs.constraints) == ROW_MUL and len(cs.z) == w_xbit[-1] + 1 + N_CMP == 521 + 2 * depth + N_CMP
    px, py = fixed_base(cs, w_xbit)
    assert len(cs.constraints) == ROW_GADGETS and len(cs.z) == 1890 + 2 * depth
    c = _hash2(cs, px, py)
    if forge is None:
        assert (cs.val(px), cs.val(py)) == bj.multiply(bj.BASE, x) and cs.z[c] == c_val
    asset = _hash2(cs, {w_amt: 1}, {w_tok: 1})
    cur = _hash2(cs, {c: 1}, {asset: 1})
    _hash2(cs, {w_x: 1}, {0: 1}, out_wire=w_nh)
    for l in range(depth):
        b, s = w_bit[l], w_sib[l]
        cs.enforce({b: 1}, {b: 1, 0: R - 1}, {})
        left = cs.alloc(cs.z[s] if cs.z[b] else cs.z[cur])
        cs.enforce({b: 1}, _lc_add({s: 1}, {cur: R - 1}), _lc_add({left: 1}, {cur: R - 1}))
        right = _lc_add({s: 1}, {cur: 1}, {left: R - 1})
        cur = _hash2(cs, {left: 1}, right, out_wire=w_root if l == depth - 1 else None)
    cs.z[w_tok] = change_token       # (a forged change_asset: the gadget's VALUES are another token's, its rows name the one token wire)
    change_asset = _hash2(cs, {w_chg: 1}, {w_tok: 1})
    cs.z[w_tok] = token
    _hash2(cs, {w_cc: 1}, {change_asset: 1}, out_wire=w_cleaf)
    assert (len(cs.z), len(cs.constraints)) == shape(depth)
    assert gadget_row(depth, 6 + depth) == len(cs.constraints)
    assert all(0 <= v < R for v in cs.z)
    return len(cs.z), N_PUB, cs.constraints, cs.z
