"""View keys for owned notes -- specification.  TEST INFRASTRUCTURE ONLY.

tests/owned_note_spec.py binds a note to a one-time key P = pk + t BASE that only the payee can spend, and its scan takes sk, the
wallet's only secret: whoever scans can spend.  A scan over the whole pool is a service by nature, so this file DEFINES the form that
separates the two powers, in plain Python over oracle/py/babyjubjub.py and oracle/py/mimc7.py: a view scalar finds and opens notes, the
spend scalar alone makes the x that the `claim` statement (tests/claim_spec.py) spends.  The product's kernels
(owshen_amd/csrc/notes.hip: og_note_seal_view_batch_d, og_note_scan_view_batch_d, og_note_unlock_batch_d) are checked against it.

With H = mimc7.hash2 (MultiMiMC7 2-to-1, key 0), mul = babyjubjub.multiply, l = ORDER / 8, small(P) <=> mul(P, 8) == (0, 1):

    keys    a view scalar v and a spend scalar sk, both canonical Fr elements; PV = mul(BASE, v), PS = mul(BASE, sk); the address is
            (PV, PS).
    KDF     from a shared point S (affine), on indices disjoint from the ordinary scheme's 1 .. 5 and the owned scheme's 6 .. 9:
            k = H(S.x, S.y); tag = H(k, 10); t = H(k, 11); pad_a = H(k, 12); pad_t = H(k, 13).  Each of the three scans answers 0 on
            the memos of the other two forms.
    seal    (e, PV, PS, amount, token):  E = mul(BASE, e), S = mul(PV, e), P = PS + mul(BASE, t), c = H(P.x, P.y),
            leaf = H(c, H(amount, token)).  memo = (E.x, E.y, tag, amount + pad_a mod r, token + pad_t mod r);  note = (c, leaf): the
            owned form's shapes, so a ledger stores them alike.
            Refused: a field >= r, amount >= 2^128, PV or PS off the curve, small(PV), small(PS), small(E), small(P).
    scan    (v, PS, memo, leaf or None): S = mul(E, v) on the integer v < r (not reduced mod l), then the KDF.  hit 0: a field >= r, E
            off the curve, small(E), or another tag.  hit 2: the tag matches and the amount is >= 2^128, or small(P), or a leaf was
            given and differs from H(c, H(amount, token)).  hit 1: the memo opens as (t, amount, token, c) with t the KDF's output,
            canonical and not reduced, and c = H(P.x, P.y) for P = PS + mul(BASE, t).  No x appears anywhere: the scanner never holds sk.
    unlock  (sk, row, leaf or None), in the wallet: x = (sk + t) mod l; the row unlocks as (x, amount, token, c) -- the opened row of
            owned_note_spec.scan_owned, the private half of a claim record -- only if the four fields are canonical, amount < 2^128,
            H(mul(BASE, x)) is the row's c and, if a leaf was given, it equals H(c, H(amount, token)).  The all-zero row a scan writes
            for a non-hit does not unlock by itself (c = 0 is the hash of no point anybody can name).

Facts:
  * The sender knows t and P but not x.
  * The view-key holder knows t, P, amount, token and c.  It does not know x, and it does not know the nullifier hash H(x, 1): it can
    find and read notes, it cannot spend them and cannot see them spent.
  * The tag depends on v alone.  Two addresses with one view key and different spend keys open each other's memos with a c that is not
    the sealed one: with a leaf this is hit 2; without a leaf the scan cannot tell, and unlock with a leaf can.
  * A PS with a torsion component seals, but the note never unlocks: x BASE lies in the prime-order subgroup and P does not.  (The
    owned form's second fact, now caught by unlock.)
  * A scanning service may withhold notes or lie about amount and token.  unlock with the leaf catches the lie; nothing catches
    withholding.
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
    return tuple(H(k, j) for j in (10, 11, 12, 13))


def leaf_of(c, amount, token):
    return H(c, H(amount, token))


def one_time_key(ps, t):
    """P = PS + t BASE"""
    return add(ps, mul(bj.BASE, t))


def seal_view(e, pv, ps, amount, token):
    """-> ((E.x, E.y, tag, enc_amount, enc_token), (c, leaf)), or None when the request is refused"""
    if max(e, pv[0], pv[1], ps[0], ps[1], amount, token) >= R or amount >= AMOUNT_BOUND:
        return None
    for q in (pv, ps):
        if not bj.is_on_curve(q) or small(q):
            return None
    big_e = mul(bj.BASE, e)
    if small(big_e):
        return None
    tag, t, pad_a, pad_t = kdf(mul(pv, e))
    p = one_time_key(ps, t)
    if small(p):
        return None
    c = H(p[0], p[1])
    return (big_e[0], big_e[1], tag, (amount + pad_a) % R, (token + pad_t) % R), (c, leaf_of(c, amount, token))


def scan_view(v, ps, memo, leaf=None):
    """-> (hit, (t, amount, token, c) or None); PS is a valid spend key (canonical, on the curve, not small): the call's business"""
    assert 0 <= v < R and max(ps) < R and bj.is_on_curve(ps) and not small(ps)
    ex, ey, tag, enc_amount, enc_token = memo
    if max(memo) >= R:
        return 0, None
    big_e = (ex, ey)
    if not bj.is_on_curve(big_e) or small(big_e):
        return 0, None
    tg, t, pad_a, pad_t = kdf(mul(big_e, v))
    if tg != tag:
        return 0, None
    amount, token = (enc_amount - pad_a) % R, (enc_token - pad_t) % R
    if amount >= AMOUNT_BOUND:
        return 2, None
    p = one_time_key(ps, t)
    if small(p):
        return 2, None
    c = H(p[0], p[1])
    if leaf is not None and leaf != leaf_of(c, amount, token):
        return 2, None
    return 1, (t, amount, token, c)


def unlock(sk, row, leaf=None):
    """-> (ok, (x, amount, token, c) or None)"""
    assert 0 <= sk < R
    t, amount, token, c = row
    if max(row) >= R or amount >= AMOUNT_BOUND:
        return 0, None
    x = (sk + t) % ELL
    p = mul(bj.BASE, x)
    if H(p[0], p[1]) != c:
        return 0, None
    if leaf is not None and leaf != leaf_of(c, amount, token):
        return 0, None
    return 1, (x, amount, token, c)
