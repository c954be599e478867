"""The transfer statement -- specification + witness generator.  TEST INFRASTRUCTURE ONLY.

No reference counterpart: the snapshot contains no circuit.  This file DEFINES the fifth statement of the pool in the
same plain form as oracle/py/withdraw.py, tests/split_spec.py and tests/join_spec.py (whose helpers it reuses); the product's builders
(owshen_amd/circuit.py transfer_r1cs, og_transfer_r1cs in keygen.hip) and the HIP witness kernels (witness.hip k_transfer_core and
k_tw9_*) are checked against it.

Statement (public: root, nullifier_hash, chain_id, pay_leaf, change_leaf; n_pub = 5):
    "I know a note under `root` worth `amount` of `token`.  It is spent.  `pay_amount` of it goes into the new leaf `pay_leaf`.  The
     rest, change = amount - pay_amount, goes into the new leaf `change_leaf`."  Nothing leaves the pool.
Private: nullifier, secret, amount, token, pay_commitment, pay_amount, change_commitment, change, the path.  `token` is ONE wire
shared by all three asset hashes; it is private, as in `join`, because nothing is paid out.  With H = MultiMiMC7 2-to-1
(oracle/py/mimc7.py):
    leaf = H(H(nullifier, secret), H(amount, token)) is under `root` at `index`;
    nullifier_hash = H(nullifier, 0);
    pay_amount + change = amount, with pay_amount < 2^128 and change < 2^128, each by a 128-bit decomposition.  The sum stays below
        2^129 < r, so it cannot wrap: this is what makes it impossible to create value;
    pay_leaf = H(pay_commitment, H(pay_amount, token));
    change_leaf = H(change_commitment, H(change, token)): both have the leaf shape of a deposit, so either note is later spent by
        `withdraw`, `split`, `join` or `transfer` like any other;
    `chain_id` is bound by its square.

Three facts about the statement:
  * `pay_commitment` and `change_commitment` are unconstrained private inputs, each a c' = H(nullifier', secret') formed off-circuit.
    The payee hands over the first one.  A c' nobody can open harms only the prover: the argument `split` already makes.
  * `pay_amount = 0` and `pay_amount = amount` are both allowed (a zero-value note on one side).
  * With it the set closes: any in-pool payment is zero or more `join`s followed by one `transfer`.

The ledger's part of a transfer, in order: verify the proof; check that `root` is known; check that `nullifier_hash` is unspent, and
mark it; append `pay_leaf`, then `change_leaf` (og_mimc7_append_d).

Wire order (the contract all implementations share):
    0 one | 1 root | 2 nullifier_hash | 3 chain_id | 4 pay_leaf | 5 change_leaf
    6 nullifier | 7 secret | 8 amount | 9 token | 10 pay_commitment | 11 pay_amount | 12 change_commitment | 13 change
    14.. siblings[D] | index bits[D] | chain_id^2 | pay_amount bits[128] (LSB first) | change bits[128]
    gadgets in the order: inner, asset, leaf, nullifier_hash (out = wire 2), level 0..D-1 (each first allocates left_l; the last
      one's out = wire 1), pay_asset = H(pay_amount, token), pay_leaf = H(pay_commitment, pay_asset) (out = wire 4), change_asset =
      H(change, token), change_leaf = H(change_commitment, change_asset) (out = wire 5)
Constraint order: chain_id^2; (pay_amount + change) * 1 = amount; for pay_amount 128 rows b (b - 1) = 0, then (sum 2^i b_i) * 1 =
pay_amount; the same 129 rows for change; the gadgets in the order above, with levels as in `split` (bit booleanity, the `left`
selector, the hash).  There are no padding gates in this statement.
"""
from oracle.py.fields import R
from oracle.py import mimc7
from oracle.py.withdraw import _CS, _hash2, _lc_add

N_PUB = 5
N_BITS = 128
ROW_SUM = 1                       # (pay_amount + change) * 1 = amount
ROW_PAY_RANGE = 2 + N_BITS        # the recomposition of pay_amount: the last of its 129 range rows
ROW_CHANGE_RANGE = 3 + 2 * N_BITS  # the recomposition of change


def shape(depth):
    """(n_wires, n_constraints): (6840, 6832) at depth 1, (7573, 7564) at 2, (29563, 29524) at 32"""
    n_wires = 267 + 3 * depth + (8 + depth) * 730
    n_constraints = 260 + 2 * depth + (8 + depth) * 730
    return n_wires, n_constraints


def gadget_row(depth, h):
    """the first row of gadget h (0 inner, 1 asset, 2 leaf, 3 nullifier_hash, 4 + l level l -- its booleanity row --, 4 + D pay_asset,
    5 + D pay_leaf, 6 + D change_asset, 7 + D change_leaf); a gadget's hash is 730 rows: 364 of the first permutation, k1, 364 of
    the second, the output"""
    return 260 + 730 * h + 2 * min(max(h - 4, 0), depth)


def leaves_of(pay_commitment, pay_amount, change_commitment, change, token):
    """the two leaves the ledger appends, in this order: (H(c_pay, H(pay_amount, token)), H(c_change, H(change, token)))"""
    return mimc7.hash2(pay_commitment, mimc7.hash2(pay_amount, token)), mimc7.hash2(change_commitment, mimc7.hash2(change, token))


def _range(cs, w_value, w_bits):
    """128 rows b (b - 1) = 0, then (sum 2^i b_i) * 1 = value"""
    for b in w_bits:
        cs.enforce({b: 1}, {b: 1, 0: R - 1}, {})
    cs.enforce({b: 1 << i for i, b in enumerate(w_bits)}, {0: 1}, {w_value: 1})


class _ForgedCS(_CS):
    """records the rows without checking them: for witnesses that are wrong on purpose (`forge`)"""

    def enforce(self, a, b, c):
        self.constraints.append((dict(a), dict(b), dict(c)))


def build(depth, nullifier, secret, amount, index, siblings, token=0, chain_id=0, pay_commitment=0, pay_amount=0, change_commitment=0,
          forge=None):
    """returns (n_wires, n_pub, constraints, witness z).
    forge = {"change": v, "pay_leaf": v, "pay_asset_token": v} (any may be missing) assembles a witness that is wrong on purpose: the
    amounts are taken as given (as field elements, `change` = amount - pay_amount mod r unless forged), wire 4 is forge["pay_leaf"],
    the wires of the pay_asset gadget are those of H(pay_amount, forge["pay_asset_token"]); every other wire follows as an honest
    prover's would -- bit wires are the low 128 bits -- and no row is checked here: the caller finds the rows that fail."""
    assert len(siblings) == depth >= 1
    forge_of = forge or {}
    if forge is None:
        assert 0 <= pay_amount <= amount < (1 << N_BITS)
    change = forge_of.get("change", (amount - pay_amount) % R)
    cs = _CS() if forge is None else _ForgedCS()
    leaf = mimc7.hash2(mimc7.hash2(nullifier, secret), mimc7.hash2(amount, token))
    root = mimc7.merkle_root_from_path(leaf, index, siblings)[-1]
    pay_token = forge_of.get("pay_asset_token", token)
    pay_leaf, change_leaf = leaves_of(pay_commitment, pay_amount, change_commitment, change, token)
    if pay_token != token:
        pay_leaf = mimc7.hash2(pay_commitment, mimc7.hash2(pay_amount, pay_token))
    w_root, w_nh, w_chain = cs.alloc(root), cs.alloc(mimc7.hash2(nullifier, 0)), cs.alloc(chain_id)
    w_pleaf, w_cleaf = cs.alloc(forge_of.get("pay_leaf", pay_leaf)), cs.alloc(change_leaf)
    w_null, w_sec, w_amt, w_tok = cs.alloc(nullifier), cs.alloc(secret), cs.alloc(amount), cs.alloc(token)
    w_pc, w_pay, w_cc, w_chg = cs.alloc(pay_commitment), cs.alloc(pay_amount), cs.alloc(change_commitment), cs.alloc(change)
    w_sib = [cs.alloc(s) for s in siblings]
    w_bit = [cs.alloc((index >> l) & 1) for l in range(depth)]
    w_csq = cs.alloc(chain_id * chain_id)
    w_pbit = [cs.alloc((pay_amount >> i) & 1) for i in range(N_BITS)]
    w_cbit = [cs.alloc((change >> i) & 1) for i in range(N_BITS)]
    cs.enforce({w_chain: 1}, {w_chain: 1}, {w_csq: 1})
    cs.enforce({w_pay: 1, w_chg: 1}, {0: 1}, {w_amt: 1})
    _range(cs, w_pay, w_pbit)
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
    cs.z[w_tok] = pay_token            # (a forged pay_asset: the gadget's VALUES are another token's, its rows name the one token wire)
    pay_asset = _hash2(cs, {w_pay: 1}, {w_tok: 1})
    cs.z[w_tok] = token
    _hash2(cs, {w_pc: 1}, {pay_asset: 1}, out_wire=w_pleaf)
    change_asset = _hash2(cs, {w_chg: 1}, {w_tok: 1})
    _hash2(cs, {w_cc: 1}, {change_asset: 1}, out_wire=w_cleaf)
    assert (len(cs.z), len(cs.constraints)) == shape(depth)
    assert gadget_row(depth, 8 + depth) == len(cs.constraints)
    assert all(0 <= v < R for v in cs.z)
    return len(cs.z), N_PUB, cs.constraints, cs.z
