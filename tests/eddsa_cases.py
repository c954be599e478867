"""Batched BabyJubJub EdDSA verification with the MiMC7 sponge against oracle/py/babyjubjub.py; shared by the
CPU-interpreter run and the GPU run."""
import collections
import functools
import random
from unittest import mock

import numpy as np

from oracle.py import babyjubjub as bj
from oracle.py import mimc7
from oracle.py.fields import R


def _rec(pk, rr, s, msg):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in (pk[0], pk[1], rr[0], rr[1], s, msg)), dtype=np.uint8).reshape(6, 32)


def case_eddsa_batch(ctx, n_valid=6, seed=1):
    rnd = random.Random(seed)
    recs, want = [], []
    # the reference's fixed-input test (babyjubjub/tests.rs:40-51: sk, randomness and message are small constants), on the real hash
    fixed = [(123456, 2345, 123456)]
    for k in range(n_valid):
        sk, rand_, msg = fixed[k] if k < len(fixed) else (rnd.randrange(1, R), rnd.randrange(R), rnd.randrange(R))
        while True:
            try:
                rr, s = bj.sign_mimc7(sk, rand_, msg)
                break
            except ValueError:   # s >= r: the reference errors out ("Invalid repr"); draw again
                rand_ = rnd.randrange(R)
        pk = bj.multiply(bj.BASE, sk)
        assert bj.verify_mimc7(pk, msg, (rr, s))
        recs.append(_rec(pk, rr, s, msg)); want.append(1)
        if k < 3:
            recs.append(_rec(pk, rr, s, (msg + 1) % R)); want.append(0)            # other message
            recs.append(_rec(pk, rr, (s + 1) % R, msg)); want.append(0)            # other s
            recs.append(_rec(pk, bj.affine_double(rr), s, msg)); want.append(0)    # other R (on the curve)
            recs.append(_rec(bj.affine_double(pk), rr, s, msg)); want.append(0)    # other key
            recs.append(_rec((pk[0], (pk[1] + 1) % R), rr, s, msg)); want.append(0)  # pk off the curve
            recs.append(_rec(pk, rr, s + R if s + R < (1 << 256) else s, msg)); want.append(0 if s + R < (1 << 256) else 1)  # non-canonical s
    # s = 0 with R = identity and h pk = identity cannot be forged without the key: identity R, s = 0 must reject for a random pk
    pk = bj.multiply(bj.BASE, 77)
    recs.append(_rec(pk, (0, 1), 0, 5)); want.append(1 if bj.verify_mimc7(pk, 5, ((0, 1), 0)) else 0)
    got = ctx.eddsa_verify(ctx.to_device(np.stack(recs)))
    assert got.tolist() == want
    for rec, w in zip(recs, want):   # the oracle agrees record by record (canonical ones)
        v = [int.from_bytes(rec[i].tobytes(), "little") for i in range(6)]
        if all(x < R for x in v):
            assert bj.verify_mimc7((v[0], v[1]), v[5], ((v[2], v[3]), v[4])) == bool(w)


# ---- a second reference, from the definition ----------------------------------------------------------------------------------
# oracle/py/babyjubjub.py restates the upstream file (projective add / double, a Z == 0 identity marker, an equality-then-double
# branch).  This one is the textbook: the affine complete addition law of a x^2 + y^2 = 1 + d x^2 y^2 (a a square, d not: no
# exceptional pairs among the curve's points) and plain double-and-add.  Every canonical record of the cases below must get the
# same decision from this, from bj.verify_mimc7 and from the kernel.
TD_A, TD_D = 168700, 168696
IDENT = (0, 1)
ELL = bj.ORDER // 8   # the prime order of BASE


def td_on_curve(p):
    x, y = p
    return (TD_A * x * x + y * y - 1 - TD_D * x * x * y * y) % R == 0


def td_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = TD_D * x1 * x2 * y1 * y2 % R
    i = pow(1 - t * t, -1, R)   # 1 / (1 + t) = (1 - t) i and 1 / (1 - t) = (1 + t) i: one inversion for the two denominators
    return ((x1 * y2 + y1 * x2) * (1 - t) * i % R, (y1 * y2 - TD_A * x1 * x2) * (1 + t) * i % R)


@functools.lru_cache(None)
def td_mul(p, k):
    acc = IDENT
    for i in reversed(range(k.bit_length())):
        acc = td_add(acc, acc)
        if (k >> i) & 1:
            acc = td_add(acc, p)
    return acc


def td_neg(p):
    return ((-p[0]) % R, p[1])


def td_order(p):
    """the order of a point of the 8-torsion (None outside it)"""
    return next((o for o in (1, 2, 4, 8) if td_mul(p, o) == IDENT), None)


def td_hash(pk, rr, msg):
    return mimc7.multi_hash([rr[0], rr[1], pk[0], pk[1], msg], 0)


def td_verify(pk, msg, rr, s):
    """the header's predicate: both points on the curve and s BASE == R + h pk (cofactorless; s is any integer)"""
    if not td_on_curve(pk) or not td_on_curve(rr):
        return False
    return td_mul(bj.BASE, s) == td_add(rr, td_mul(pk, td_hash(pk, rr, msg)))


_bj_multiply = functools.lru_cache(None)(bj.multiply)   # memoised: keys, nonces and s BASE repeat across records


def sign_with_nonce(sk, pk, r, msg, rr=None):
    """(R = r BASE, s = (r + h sk) mod ORDER) with the nonce given (bj.sign_mimc7 derives it from a hash and cannot reach the edge
    nonces); `pk` is hashed as given, so a key with a low-order component can be signed over.  s >= r raises as the oracle does.
    `rr` publishes (and hashes) another R than r BASE: a forgery attempt whose s still answers the nonce."""
    rr = _bj_multiply(bj.BASE, r) if rr is None else rr
    s = (r + td_hash(pk, rr, msg) * sk) % bj.ORDER
    if s >= R:
        raise ValueError("Invalid repr")
    return rr, s


def low_order_points(rnd):
    """T2 = (0, -1), T4 = (1 / sqrt a, 0), T8 = ELL P for a random curve point P: derived, and their orders asserted"""
    t2 = (0, R - 1)
    ra = bj.fr_sqrt(TD_A)
    assert ra is not None and ra * ra % R == TD_A
    t4 = (pow(ra, -1, R), 0)
    while True:
        x = rnd.randrange(R)
        y = bj.fr_sqrt((1 - TD_A * x * x) * pow(1 - TD_D * x * x, -1, R) % R)
        if y is None:
            continue
        assert y * y % R == (1 - TD_A * x * x) * pow(1 - TD_D * x * x, -1, R) % R and td_on_curve((x, y))
        t8 = td_mul((x, y), ELL)
        if td_mul(t8, 4) != IDENT:
            break
    for t, o in ((t2, 2), (t4, 4), (t8, 8)):
        assert td_on_curve(t) and td_order(t) == o and td_mul(t, o // 2) != IDENT
    assert td_mul(bj.BASE, ELL) == IDENT and td_order(bj.BASE) is None
    return t2, t4, t8


# class: the record class of the issue (1..9; 0 = the pool's random part), expect: the decision that the class's reasoning
# predicts (None: "whatever the references say")
Rec = collections.namedtuple("Rec", "cls tag pk rr s msg expect")
BOTH_OUTCOMES = (1, 2, 3, 4, 5, 8)     # classes that must show an accept and a reject
ONE_OUTCOME = {6: 0, 7: 0, 9: 1}
POOL = 193                             # prime: a tiled pool never lines up with the 64-lane grid


def _valid(rnd, sk, pk, nonce=None, msg=None):
    """a valid (pk, R, s, msg); whatever is not given is drawn, again while s >= r"""
    while True:
        k = rnd.randrange(1, ELL) if nonce is None else nonce
        m = rnd.randrange(R) if msg is None else msg
        try:
            rr, s = sign_with_nonce(sk, pk, k, m)
        except ValueError:
            if nonce is not None and msg is not None:
                raise
            continue
        return pk, rr, s, m


@functools.lru_cache(None)
def edge_records():
    rnd = random.Random(0xEDD5A)
    t2, t4, t8 = low_order_points(rnd)
    torsion = (("T2", t2, 2), ("T4", t4, 4), ("T8", t8, 8))
    out = []

    def key():
        sk = rnd.randrange(1, ELL)
        return sk, _bj_multiply(bj.BASE, sk)

    # 1. s outside the subgroup range: s + k ELL is the same multiple of BASE; s +- 1 is not
    sk, pk = key()
    pk, rr, s, m = _valid(rnd, sk, pk)
    for k in range(-8, 9):
        if k and 0 <= s + k * ELL < R:
            out.append(Rec(1, f"s{k:+d}l", pk, rr, s + k * ELL, m, 1))
    out.append(Rec(1, "s+1", pk, rr, (s + 1) % R, m, 0))
    out.append(Rec(1, "s-1", pk, rr, (s - 1) % R, m, 0))
    # 2. mixed-order keys pk' = sk BASE + T, signed with sk over pk': s BASE == R + h sk BASE + h T  <=>  ord(T) | h
    for name, t, o in torsion:
        sk, pk = key()
        pk = td_add(pk, t)
        nonce, seen = rnd.randrange(1, ELL), set()
        rr = _bj_multiply(bj.BASE, nonce)
        for m in range(200):
            acc = td_hash(pk, rr, m) % o == 0
            if acc not in seen:
                seen.add(acc)
                out.append(Rec(2, f"pk+{name}", *_valid(rnd, sk, pk, nonce, m), int(acc)))
            if len(seen) == 2:
                break
        assert len(seen) == 2
    # 3. low-order and identity keys, R = r BASE, s = r: accepts  <=>  h pk is the identity  <=>  ord(pk) | h
    for name, t, o in (("O", IDENT, 1),) + torsion:
        nonce, seen = rnd.randrange(1, ELL), collections.Counter()
        rr = _bj_multiply(bj.BASE, nonce)
        for m in range(200):
            acc = td_hash(t, rr, m) % o == 0
            if seen[acc] < (3 if o == 1 else 1):
                seen[acc] += 1
                out.append(Rec(3, f"pk={name}", t, rr, nonce, m, int(acc)))
            if sum(seen.values()) == (3 if o == 1 else 2):
                break
        assert len(seen) == (1 if o == 1 else 2)
    # 4. R with a low-order component: R + T leaves the subgroup, s BASE never does; R = identity is the nonce 0
    sk, pk = key()
    pk, rr, s, m = _valid(rnd, sk, pk)
    for name, t, o in torsion:
        out.append(Rec(4, f"R+{name}", pk, td_add(rr, t), s, m, 0))
    pk, rr, s, m = _valid(rnd, sk, pk, nonce=0)
    assert rr == IDENT
    out.append(Rec(4, "R=O", pk, rr, s, m, 1))
    # 5. an accumulator at or near the identity: pk = BASE (BASE - pk is the identity; s = nonce + h), pk = -BASE, pk = 2 BASE
    for name, sk, pk, nonces in (("B", 1, bj.BASE, (0, 1, 2, 3)), ("-B", ELL - 1, td_neg(bj.BASE), (5,)),
                                 ("2B", 2, td_add(bj.BASE, bj.BASE), (rnd.randrange(1, ELL),))):
        assert _bj_multiply(bj.BASE, sk) == pk
        for nonce in nonces:
            pk, rr, s, m = _valid(rnd, sk, pk, nonce=nonce)
            tag = f"pk={name},nonce={nonce if nonce < 9 else 'random'}"
            out.append(Rec(5, tag, pk, rr, s, m, 1))
            out.append(Rec(5, tag + ",msg^1", pk, rr, s, m ^ 1, 0))
    # 6. sign flips, all on the curve.  The last one is the record for a comparison that drops a coordinate: flipping R.y of a
    # finished signature changes h, and s BASE - h pk lands nowhere near R; so the flipped R is published and hashed BEFORE s is
    # computed, s still answers the nonce, and s BASE - h pk = nonce BASE = (R.x, -R.y): equal to R in x, different in y.
    sk, pk = key()
    pk, rr, s, m = _valid(rnd, sk, pk)
    out.append(Rec(6, "-R.x", pk, ((-rr[0]) % R, rr[1]), s, m, 0))
    out.append(Rec(6, "-R.y", pk, (rr[0], (-rr[1]) % R), s, m, 0))
    out.append(Rec(6, "-pk.x", ((-pk[0]) % R, pk[1]), rr, s, m, 0))
    nonce = rnd.randrange(1, ELL)
    nb = _bj_multiply(bj.BASE, nonce)
    flipped = (nb[0], (-nb[1]) % R)
    _, s2 = sign_with_nonce(sk, pk, nonce, m, rr=flipped)
    assert td_add(td_mul(bj.BASE, s2), td_neg(td_mul(pk, td_hash(pk, flipped, m)))) == nb
    out.append(Rec(6, "sB-hpk=(R.x,-R.y)", pk, flipped, s2, m, 0))
    assert all(td_on_curve(r.pk) and td_on_curve(r.rr) for r in out[-4:])
    # 7. R off the curve
    out.append(Rec(7, "R.y+1", pk, (rr[0], (rr[1] + 1) % R), s, m, 0))
    assert not td_on_curve(out[-1].rr)
    # 8. non-canonical encodings, field by field (Rec holds the six integers as they are encoded)
    sk, pk = key()
    pk, rr, s, m = _valid(rnd, sk, pk)
    out.append(Rec(8, "canonical", pk, rr, s, m, 1))
    v = [pk[0], pk[1], rr[0], rr[1], s, m]
    for k, name in enumerate(("pk.x", "pk.y", "R.x", "R.y", "s", "msg")):
        for what, bad in (("+r", v[k] + R), ("=2^256-1", (1 << 256) - 1)):
            if bad < 1 << 256:
                w = v[:k] + [bad] + v[k + 1:]
                out.append(Rec(8, name + what, (w[0], w[1]), (w[2], w[3]), w[4], w[5], 0))
    # 9. message extremes
    for m in (0, R - 1):
        sk, pk = key()
        out.append(Rec(9, f"msg={'0' if m == 0 else 'r-1'}", *_valid(rnd, sk, pk, msg=m), 1))
    return tuple(out)


@functools.lru_cache(None)
def pool_records():
    """POOL distinct records: the edge records, then honest random signatures under a few keys, each followed by one corruption"""
    rnd = random.Random(0x193)
    out = list(edge_records())
    keys = [rnd.randrange(1, ELL) for _ in range(6)]
    prev, j = None, 0
    while len(out) < POOL:
        if j % 2 == 0:
            sk = keys[(j // 2) % len(keys)]
            prev = _valid(rnd, sk, _bj_multiply(bj.BASE, sk))
            out.append(Rec(0, "honest", *prev, 1))
        else:
            pk, rr, s, m = prev
            kind = (j // 2) % 6
            bad = ((pk, rr, s, (m + 1) % R), (pk, rr, (s + 1) % R, m), (pk, td_add(rr, rr), s, m), (td_add(pk, pk), rr, s, m),
                   ((pk[0], (pk[1] + 1) % R), rr, s, m), (pk, out[-3].rr if out[-3].cls == 0 else td_neg(rr), s, m))[kind]
            out.append(Rec(0, "corrupt%d" % kind, *bad, 0))
        j += 1
    assert len(out) == POOL and len({r[2:6] for r in out}) == POOL
    return tuple(out)


def canonical(rec):
    return all(v < R for v in (*rec.pk, *rec.rr, rec.s, rec.msg))


@functools.lru_cache(None)
def decide(rec):
    """the expected decision of one record, computed once per session: both references for a canonical record (and the class's
    prediction where it makes one), 0 for a non-canonical one (the header's rule; the only records without a reference decision)"""
    if not canonical(rec):
        assert rec.expect == 0
        return 0
    d_td = td_verify(rec.pk, rec.msg, rec.rr, rec.s)
    with mock.patch.object(bj, "multiply", _bj_multiply):   # the oracle's own multiply, memoised: records share s BASE or h pk
        d_bj = bj.verify_mimc7(rec.pk, rec.msg, (rec.rr, rec.s))
    assert d_td == d_bj, f"the two references disagree on {rec.cls}:{rec.tag}: definition {d_td}, oracle {d_bj}"
    assert rec.expect is None or rec.expect == d_td, f"{rec.cls}:{rec.tag}: predicted {rec.expect}, references {d_td}"
    return int(d_td)


def records_array(recs):
    if not recs:
        return np.zeros((0, 6, 32), dtype=np.uint8)
    return np.stack([_rec(r.pk, r.rr, r.s, r.msg) for r in recs])


def class_census(recs):
    """{class: [rejects, accepts]} and the number of records exempted from the reference decision"""
    census = collections.defaultdict(lambda: [0, 0])
    for r in recs:
        census[r.cls][decide(r)] += 1
    return dict(census), sum(not canonical(r) for r in recs)


def check_edge_coverage(recs):
    census, exempt = class_census(recs)
    for c in BOTH_OUTCOMES:
        assert census[c][0] and census[c][1], f"class {c} shows one outcome only: {census[c]}"
    for c, w in ONE_OUTCOME.items():
        assert census[c][w] and not census[c][1 - w], f"class {c}: {census[c]}"
    # the exempted records are the non-canonical encodings of class 8 and nothing else
    assert exempt == sum(r.cls == 8 and r.tag != "canonical" for r in recs) and exempt >= 6
    assert all(canonical(r) for r in recs if r.cls != 8)
    return census, exempt


def _assert_decisions(got, want, names):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "wrong decisions (lane: record got/want): " + ", ".join(
        f"{i}: {names(i)} {got[i]}/{want[i]}" for i in bad[:12]) + (" ..." if bad.size > 12 else "")


def case_eddsa_edges(ctx, keep=None):
    """one call over the edge records (`keep`: a filter for a runner that cannot afford them all; the coverage rules still hold)"""
    recs = [r for r in edge_records() if keep is None or keep(r)]
    census, exempt = check_edge_coverage(recs)
    want = np.array([decide(r) for r in recs], dtype=np.uint32)
    got = ctx.eddsa_verify(ctx.to_device(records_array(recs)))
    print("eddsa edges: %d records, {class: [rejects, accepts]} = %s, %d exempt from the references" % (len(recs), census, exempt))
    _assert_decisions(got, want, lambda i: f"{recs[i].cls}:{recs[i].tag}")


@functools.lru_cache(None)
def pool(m=POOL):
    """(records [m, 6, 32], decisions [m]) of the pool's first m records, read-only"""
    recs = pool_records()[:m]
    arr, want = records_array(recs), np.array([decide(r) for r in recs], dtype=np.uint32)
    assert all(canonical(r) for r in recs if r.cls != 8)   # nothing but class 8's encodings goes without a reference decision
    if m == POOL:
        assert 0.4 <= want.mean() <= 0.6, want.mean()
    arr.setflags(write=False)
    want.setflags(write=False)
    return arr, want


def tiled(n, m=POOL, off=0):
    """record i of a call of n is pool[(7 i + n + off) mod m]: lanes are independent, so this tests the index, stride and bound"""
    arr, want = pool(m)
    idx = (np.arange(n, dtype=np.int64) * 7 + n + off) % m
    return arr[idx], want[idx], idx


def other_offset(n, m=POOL):
    """the first offset whose expectation differs from offset 0's in the call's LAST lane: a lane that is never written keeps one
    value over both calls and fails one of them, whatever the buffer held"""
    _, want = pool(m)
    return next(off for off in range(1, m) if want[(7 * (n - 1) + n + off) % m] != want[(7 * (n - 1) + n) % m])


def case_eddsa_shapes(ctx, sizes, reuse=(), m=POOL):
    """every size twice (offset 0 and other_offset), then the `reuse` sizes in turn with an offset of their position: the result
    buffer is one arena entry reused across calls of different n"""
    names = pool_records()
    calls = [(n, off) for n in sizes for off in ((0, other_offset(n, m)) if n else (0,))]
    calls += [(n, 11 * k) for k, n in enumerate(reuse)]
    for n, off in calls:
        arr, want, idx = tiled(n, m, off)
        got = ctx.eddsa_verify(ctx.to_device(arr))
        assert isinstance(got, np.ndarray) and got.shape == (n,)
        _assert_decisions(got, want, lambda i: f"n={n} off={off} {names[idx[i]].cls}:{names[idx[i]].tag}")
