"""The split statement -- specification + witness generator.  TEST INFRASTRUCTURE ONLY.

No reference counterpart: the snapshot's withdraw is an ECDSA-authorised burn of a whole amount
(``/root/reference/src/services/api_services/withdraw.rs:27-71``) and contains no circuit.  This file DEFINES the
third statement of the pool in the same plain form as oracle/py/withdraw.py and oracle/py/deposit.py (whose helpers it reuses);
the product's builders (owshen_amd/circuit.py split_r1cs, og_split_r1cs in keygen.hip) and the HIP witness kernel (witness.hip
k_split_core) are checked against it.

Statement (public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf; n_pub = 7):
    "I know a note under `root` worth `amount` of `token`.  I take `amount_out` of it out to `recipient`.  The rest,
     change = amount - amount_out, goes into the new leaf `change_leaf`."
Private: nullifier, secret, amount, change_commitment, change, the path.  With H = MultiMiMC7 2-to-1 (oracle/py/mimc7.py):
    leaf = H(H(nullifier, secret), H(amount, token)) is under `root` at `index`;
    nullifier_hash = H(nullifier, 0);
    amount_out + change = amount, with amount_out < 2^128 and change < 2^128, each by a 128-bit decomposition.  The sum stays
        below 2^129 < r, so it cannot wrap: this is what stops an overdraw;
    change_leaf = H(change_commitment, H(change, token)): the leaf shape of a deposit, so the change note is later spent by
        `withdraw` or `split` like any other;
    `recipient` and `chain_id` are bound by a square each, as in `withdraw`.

Three facts about the statement:
  * `amount` is private here.  The input note's size is no longer revealed; only `amount_out` is.
  * `change_commitment` is an unconstrained private input.  The prover forms c' = H(nullifier', secret') off-circuit.  A c' nobody
    can open harms only the prover, which is the argument of oracle/py/deposit.py.
  * `amount_out = 0` with somebody else's c' is an in-pool transfer.  `amount_out = amount` leaves a zero-value change note.

The ledger's part of a split, in order: verify the proof; check that `root` is known; check that `nullifier_hash` is unspent; pay
`amount_out`; append `change_leaf` (og_mimc7_append_d).

Wire order (the contract all implementations share):
    0 one | 1 root | 2 nullifier_hash | 3 recipient | 4 amount_out | 5 token | 6 chain_id | 7 change_leaf
    8 nullifier | 9 secret | 10 amount | 11 change_commitment | 12 change
    13.. siblings[D] | index bits[D] | recipient^2 | chain_id^2 | amount_out bits[128] (LSB first) | change bits[128]
    gadgets in the order: inner, asset, leaf, nullifier_hash (out = wire 2), level 0..D-1 (each first allocates left_l; the last
      one's out = wire 1), change_asset = H(change, token), change_leaf = H(change_commitment, change_asset) (out = wire 7)
Constraint order: recipient^2; chain_id^2; (amount_out + change) * 1 = amount; for amount_out 128 rows b (b - 1) = 0, then
(sum 2^i b_i) * 1 = amount_out; the same 129 rows for change; the gadgets in the order above, with levels as in `withdraw` (bit
booleanity, the `left` selector, the hash).  There are no padding gates in this statement.
"""
from oracle.py.fields import R
from oracle.py import mimc7
from oracle.py.withdraw import _CS, _hash2, _lc_add

N_PUB = 7
N_BITS = 128


def shape(depth):
    """(n_wires, n_constraints): (5381, 5373) at depth 1, (6114, 6105) at 2, (28104, 28065) at 32"""
    n_wires = 1 + 7 + 5 + 2 * depth + 2 + 256 + depth + (6 + depth) * 730 - 3
    n_constraints = 3 + 258 + 2 * depth + (6 + depth) * 730
    return n_wires, n_constraints


def change_leaf_of(change_commitment, change, token):
    """the leaf the ledger appends for the change note: H(c', H(change, token))"""
    return mimc7.hash2(change_commitment, mimc7.hash2(change, token))


def _range(cs, w_value, w_bits):
    """128 rows b (b - 1) = 0, then (sum 2^i b_i) * 1 = value"""
    for b in w_bits:
        cs.enforce({b: 1}, {b: 1, 0: R - 1}, {})
    cs.enforce({b: 1 << i for i, b in enumerate(w_bits)}, {0: 1}, {w_value: 1})


def build(depth, nullifier, secret, amount, recipient, amount_out, index, siblings, token=0, chain_id=0, change_commitment=0):
    """returns (n_wires, n_pub, constraints, witness z)."""
    assert len(siblings) == depth >= 1
    assert 0 <= amount_out <= amount < (1 << N_BITS)
    change = amount - amount_out
    cs = _CS()
    leaf = mimc7.hash2(mimc7.hash2(nullifier, secret), mimc7.hash2(amount, token))
    root = mimc7.merkle_root_from_path(leaf, index, siblings)[-1]
    w_root, w_nh = cs.alloc(root), cs.alloc(mimc7.hash2(nullifier, 0))
    w_rec, w_out, w_tok, w_chain = cs.alloc(recipient), cs.alloc(amount_out), cs.alloc(token), cs.alloc(chain_id)
    w_cleaf = cs.alloc(change_leaf_of(change_commitment, change, token))
    w_null, w_sec, w_amt = cs.alloc(nullifier), cs.alloc(secret), cs.alloc(amount)
    w_cc, w_chg = cs.alloc(change_commitment), cs.alloc(change)
    w_sib = [cs.alloc(s) for s in siblings]
    w_bit = [cs.alloc((index >> l) & 1) for l in range(depth)]
    w_rsq = cs.alloc(recipient * recipient)
    w_csq = cs.alloc(chain_id * chain_id)
    w_obit = [cs.alloc((amount_out >> i) & 1) for i in range(N_BITS)]
    w_cbit = [cs.alloc((change >> i) & 1) for i in range(N_BITS)]
    cs.enforce({w_rec: 1}, {w_rec: 1}, {w_rsq: 1})
    cs.enforce({w_chain: 1}, {w_chain: 1}, {w_csq: 1})
    cs.enforce({w_out: 1, w_chg: 1}, {0: 1}, {w_amt: 1})
    _range(cs, w_out, w_obit)
    _range(cs, w_chg, w_cbit)
    inner = _hash2(cs, {w_null: 1}, {w_sec: 1})
    asset = _hash2(cs, {w_amt: 1}, {w_tok: 1})
    cur = _hash2(cs, {inner: 1}, {asset: 1})
    assert cs.z[cur] == leaf
    _hash2(cs, {w_null: 1}, {}, out_wire=w_nh)
    for l in range(depth):
        b, s = w_bit[l], w_sib[l]
        cs.enforce({b: 1}, {b: 1, 0: R - 1}, {})
        left = cs.alloc(cs.z[s] if cs.z[b] else cs.z[cur])
        cs.enforce({b: 1}, _lc_add({s: 1}, {cur: R - 1}), _lc_add({left: 1}, {cur: R - 1}))
        right = _lc_add({s: 1}, {cur: 1}, {left: R - 1})
        cur = _hash2(cs, {left: 1}, right, out_wire=w_root if l == depth - 1 else None)
    change_asset = _hash2(cs, {w_chg: 1}, {w_tok: 1})
    _hash2(cs, {w_cc: 1}, {change_asset: 1}, out_wire=w_cleaf)
    assert (len(cs.z), len(cs.constraints)) == shape(depth)
    assert all(0 <= v < R for v in cs.z)
    return len(cs.z), N_PUB, cs.constraints, cs.z
