"""Owned notes -- specification.  TEST INFRASTRUCTURE ONLY.

tests/note_spec.py seals a note whose spending secrets are nullifier' = H(k, 2) and secret' = H(k, 3) with k = H(S), S = e pk = sk E.
The sender chose e, so the sender knows S, k and both secrets: whoever pays such a note can spend it before the payee does, and can
watch for its nullifier hash.  This file DEFINES the form that closes the hole, in plain Python over oracle/py/babyjubjub.py and
oracle/py/mimc7.py: the note is bound to a one-time public key P = pk + t BASE whose discrete logarithm x = sk + t mod l only the
payee knows, and it is spent by the `claim` statement (tests/claim_spec.py), which proves knowledge of x.  The product's kernels
(owshen_amd/csrc/notes.hip: og_note_seal_owned_batch_d, og_note_scan_owned_batch_d) are checked against it.

With H = mimc7.hash2 (MultiMiMC7 2-to-1, key 0), mul = babyjubjub.multiply, l = ORDER / 8, small(P) <=> mul(P, 8) == (0, 1):

    KDF     from a shared point S (affine), on indices disjoint from the ordinary scheme's 1 .. 5: k = H(S.x, S.y); tag = H(k, 6);
            t = H(k, 7); pad_a = H(k, 8); pad_t = H(k, 9).  Because the indices are disjoint, an ordinary scan answers 0 for an owned
            memo and an owned scan answers 0 for an ordinary one.
    seal    (e, pk, amount, token):  E = mul(BASE, e), S = mul(pk, e), P = pk + mul(BASE, t), c = H(P.x, P.y),
            leaf = H(c, H(amount, token)) -- the pool's leaf shape with c in the commitment's place.
            memo = (E.x, E.y, tag, amount + pad_a mod r, token + pad_t mod r);  note = (c, leaf).
            Refused: what the ordinary seal refuses (a field >= r, amount >= 2^128, pk off the curve, small(pk), small(E)), and small(P).
    scan    (sk, memo, leaf or None): S = mul(E, sk), then the KDF.  hit 0 and hit 2 have the ordinary scan's meaning; hit 1 opens the
            memo as (x, amount, token, c) with x = (sk + t) mod l, written canonically, and c = H(P.x, P.y) for P = mul(BASE, x).  When
            a leaf is given it is compared with H(c, H(amount, token)); a difference is hit 2.

Two facts:
  * A sender who reuses e for the same pk makes two notes with one x.  Their nullifier hash H(x, 1) is the same, so only one of them
    can be claimed.  The loss is the sender's: the payee is paid once and loses nothing that was theirs.
  * A pk with a torsion component can never be claimed: P = pk + t BASE then lies outside the prime-order subgroup, x BASE does not,
    so the c of the scan differs from the c of the seal (with a leaf beside the memo the scan answers 2).  The fault lies with the
    key's owner, who published a key that is not sk BASE.
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


def add(p, q):
    """the complete affine law (oracle/py/babyjubjub.affine_add doubles equal points by another formula: the same point)"""
    return bj.affine_add(p, q)


def kdf(s):
    """S -> (tag, t, pad_a, pad_t)"""
    k = H(s[0], s[1])
    return tuple(H(k, j) for j in (6, 7, 8, 9))


def leaf_of(c, amount, token):
    return H(c, H(amount, token))


def one_time_key(pk, t):
    """P = pk + t BASE"""
    return add(pk, mul(bj.BASE, t))


def seal_owned(e, pk, amount, token):
    """-> ((E.x, E.y, tag, enc_amount, enc_token), (c, leaf)), or None when the request is refused"""
    if max(e, pk[0], pk[1], amount, token) >= R or amount >= AMOUNT_BOUND:
        return None
    if not bj.is_on_curve(pk) or small(pk):
        return None
    big_e = mul(bj.BASE, e)
    if small(big_e):
        return None
    tag, t, pad_a, pad_t = kdf(mul(pk, e))
    p = one_time_key(pk, t)
    if small(p):
        return None
    c = H(p[0], p[1])
    return (big_e[0], big_e[1], tag, (amount + pad_a) % R, (token + pad_t) % R), (c, leaf_of(c, amount, token))


def scan_owned(sk, memo, leaf=None):
    """-> (hit, (x, amount, token, c) or None)"""
    assert 0 <= sk < R
    ex, ey, tag, enc_amount, enc_token = memo
    if max(memo) >= R:
        return 0, None
    big_e = (ex, ey)
    if not bj.is_on_curve(big_e) or small(big_e):
        return 0, None
    tg, t, pad_a, pad_t = kdf(mul(big_e, sk))
    if tg != tag:
        return 0, None
    amount, token = (enc_amount - pad_a) % R, (enc_token - pad_t) % R
    if amount >= AMOUNT_BOUND:
        return 2, None
    x = (sk + t) % ELL
    p = mul(bj.BASE, x)
    c = H(p[0], p[1])
    if leaf is not None and leaf != leaf_of(c, amount, token):
        return 2, None
    return 1, (x, amount, token, c)
