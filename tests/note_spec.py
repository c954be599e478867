"""Stealth notes -- specification.  TEST INFRASTRUCTURE ONLY.

No reference counterpart: the snapshot has the curve (oracle/py/babyjubjub.py restates its file) and no payment scheme.  This file
DEFINES how a note is sealed to a public key and how a wallet finds and opens its notes, in plain Python over oracle/py/babyjubjub.py
and oracle/py/mimc7.py; the product's kernels (owshen_amd/csrc/notes.hip: og_note_seal_batch_d, og_note_scan_batch_d) are checked
against it.

With H = mimc7.hash2 (MultiMiMC7 2-to-1, key 0), mul = babyjubjub.multiply, l the order of BASE, small(P) <=> mul(P, 8) == (0, 1):

    keys    sk: any canonical Fr element.  pk = mul(BASE, sk).
    KDF     from a shared point S (affine): k = H(S.x, S.y); tag = H(k, 1); nullifier' = H(k, 2); secret' = H(k, 3); pad_a = H(k, 4);
            pad_t = H(k, 5).
    seal    (e, pk, amount, token):  E = mul(BASE, e), S = mul(pk, e), c' = H(nullifier', secret'), leaf = H(c', H(amount, token)) --
            the leaf shape of every statement of the pool.
            memo = (E.x, E.y, tag, amount + pad_a mod r, token + pad_t mod r);  note = (c', leaf).
            Refused: a field >= r, amount >= 2^128, pk off the curve, small(pk), small(E) (i.e. e = 0 mod l).
    scan    (sk, memo, leaf or None): S = mul(E, sk), then the KDF.
            0   a field >= r, E off the curve, small(E), or the tag differs: not this wallet's.  Memos come from anybody: a malformed
                memo is never an error.
            2   the tag matches and the memo does not open: the decrypted amount is >= 2^128, or a leaf was given and the recomputed
                one differs.  Hostile or broken; the wallet ignores it.
            1   the payee's: opened as (nullifier', secret', amount, token).

Two facts:
  * small(E) is refused because E = (0, 1) gives S = (0, 1) for every sk: every wallet of the world would see its own tag.
  * sk is not reduced mod l.  E may be a point of the prime-order subgroup plus torsion, and then sk and sk mod l give different S.
    The scheme follows `multiply` on the integer sk < r.  (For an honest E = e BASE the two agree, so the key of sk + l opens what
    was sealed to the key of sk: they are the same public key.)
"""
from oracle.py import babyjubjub as bj
from oracle.py import mimc7
from oracle.py.fields import R

ELL = bj.ORDER // 8
AMOUNT_BOUND = 1 << 128
IDENTITY = (0, 1)
H = mimc7.hash2
mul = bj.multiply


def small(p):
    return mul(p, 8) == IDENTITY


def kdf(s):
    """S -> (tag, nullifier', secret', pad_a, pad_t)"""
    k = H(s[0], s[1])
    return tuple(H(k, j) for j in (1, 2, 3, 4, 5))


def leaf_of(commitment, amount, token):
    return H(commitment, H(amount, token))


def seal(e, pk, amount, token):
    """-> ((E.x, E.y, tag, enc_amount, enc_token), (c', leaf)), or None when the request is refused"""
    if max(e, pk[0], pk[1], amount, token) >= R or amount >= AMOUNT_BOUND:
        return None
    if not bj.is_on_curve(pk) or small(pk):
        return None
    big_e = mul(bj.BASE, e)
    if small(big_e):
        return None
    tag, nullifier, secret, pad_a, pad_t = kdf(mul(pk, e))
    c = H(nullifier, secret)
    return (big_e[0], big_e[1], tag, (amount + pad_a) % R, (token + pad_t) % R), (c, leaf_of(c, amount, token))


def scan(sk, memo, leaf=None):
    """-> (hit, (nullifier', secret', amount, token) or None)"""
    assert 0 <= sk < R
    ex, ey, tag, enc_amount, enc_token = memo
    if max(memo) >= R:
        return 0, None
    big_e = (ex, ey)
    if not bj.is_on_curve(big_e) or small(big_e):
        return 0, None
    t, nullifier, secret, pad_a, pad_t = kdf(mul(big_e, sk))
    if t != tag:
        return 0, None
    amount, token = (enc_amount - pad_a) % R, (enc_token - pad_t) % R
    if amount >= AMOUNT_BOUND:
        return 2, None
    if leaf is not None and leaf != leaf_of(H(nullifier, secret), amount, token):
        return 2, None
    return 1, (nullifier, secret, amount, token)
