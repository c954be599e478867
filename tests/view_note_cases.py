"""View keys on the device -- og_note_seal_view_batch_d, og_note_scan_view_batch_d, og_note_unlock_batch_d -- against
tests/view_note_spec.py (plain Python over oracle/py/babyjubjub.py and oracle/py/mimc7.py); shared by the CPU-interpreter run
(tests/test_emu_view_notes.py) and the GPU run (tests/test_gpu_view_notes.py).  The edge inputs are those of the owned pair
(tests/owned_note_cases.py), with what the view form adds: a second point in the request, a spend key as an argument of the scan, the
other two forms' memos in one pool, one view key under two spend keys, and rows that wrap sk + t past l every number of times.

Layouts (include/owshen_gpu.h): seal request = e | PV.x | PV.y | PS.x | PS.y | amount | token; memo = E.x | E.y | tag | amount + pad_a |
token + pad_t; note = c | leaf; opened row = t | amount | token | c; unlocked row = x | amount | token | c.  Every expected value is
computed once per session from the spec and handed out read-only.  Every comparison is byte equality."""
import functools
import random
from unittest import mock

import numpy as np

from oracle.py import babyjubjub as bj
from oracle.py import mimc7
from oracle.py.fields import R
from tests import note_cases as nc
from tests import note_spec
from tests import owned_note_cases as oc
from tests import owned_note_spec
from tests import view_note_spec as spec
from tests.eddsa_keys_cases import POOL, _bytes, _host, _ints, _same

ELL = spec.ELL
_mul = nc._mul
_frozen = nc._frozen
TOP_AMOUNT = nc.TOP_AMOUNT
TOP_MULTIPLE = R // ELL * ELL   # the largest multiple of l below r: 7 l


def _spec_memo():
    return mock.patch.object(spec, "mul", _mul)


def view_keys():
    """(v, PV): the owned cases' scanning keys -- a random one not below l first, three others, r - 1, l - 1, l + 1 and 2 l + 1"""
    return oc.scan_keys()


@functools.lru_cache(None)
def spend_keys():
    """(sk, PS): the wallet's, and a second wallet's that shares the view key"""
    rnd = random.Random(0x5BE2D)
    return tuple((k, _mul(bj.BASE, k)) for k in (rnd.randrange(ELL, R), rnd.randrange(1, R)))


def _expect_error(call, *words):
    from owshen_amd.api import OwshenGpuError
    try:
        call()
    except OwshenGpuError as e:
        assert e.code == -1 and all(w in str(e) for w in words), e
    else:
        raise AssertionError(f"accepted: {words}")


# ---- seal ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seal_requests():
    """((tag, (e, PV.x, PV.y, PS.x, PS.y, amount, token), refused), ...): each refusal of the issue on its own"""
    rnd = random.Random(0x71E3)
    keys, (_, ps), (_, ps2) = view_keys(), *spend_keys()
    pv = keys[0][1]
    good = (rnd.randrange(1, R), *pv, *ps, rnd.randrange(1 << 64), rnd.randrange(1 << 160))
    out = [("random", (rnd.randrange(1, R), *keys[i % 4][1], *(ps, ps2)[i & 1], rnd.randrange(1 << 100), rnd.randrange(R)), False) for i in range(8)]
    out += [("e=r-1", (R - 1, *good[1:]), False), ("amount=0", (*good[:5], 0, good[6]), False),
            ("amount=2^128-1", (*good[:5], TOP_AMOUNT, good[6]), False), ("token=r-1", (*good[:6], R - 1), False),
            ("PV = PS", (good[0], *ps, *ps, *good[5:]), False)]
    for k, name in enumerate(("e", "PV.x", "PV.y", "PS.x", "PS.y", "amount", "token")):
        out.append((name + "=r", good[:k] + (R,) + good[k + 1:], True))
    out.append(("all ff", good[:6] + ((1 << 256) - 1,), True))
    out.append(("amount=2^128", (*good[:5], 1 << 128, good[6]), True))
    out.append(("PV off the curve", (good[0], pv[0], (pv[1] + 1) % R, *good[3:]), True))
    out.append(("PS off the curve", (*good[:3], ps[0], (ps[1] + 1) % R, *good[5:]), True))
    for t in nc.torsion():
        out.append((f"PV of order {nc._order(t)}", (good[0], *t, *good[3:]), True))
        out.append((f"PS of order {nc._order(t)}", (*good[:3], *t, *good[5:]), True))
    out += [("e=0", (0, *good[1:]), True), ("e=l", (ELL, *good[1:]), True), ("e=2l", (2 * ELL, *good[1:]), True)]
    t8 = nc.torsion()[1]   # a mixed-order point is no reason to refuse, in either place
    out.append(("PV + T8", (good[0], *bj.affine_add(pv, t8), *good[3:]), False))
    out.append(("PS + T8", (*good[:3], *bj.affine_add(ps, t8), *good[5:]), False))
    return tuple(out)


@functools.lru_cache(None)
def _seal_expect(reqs):
    memos, notes, ok = [], [], []
    with _spec_memo():
        for e, vx, vy, sx, sy, amount, token in reqs:
            got = spec.seal_view(e, (vx, vy), (sx, sy), amount, token)
            memos.append(got[0] if got else (0,) * 5)
            notes.append(got[1] if got else (0,) * 2)
            ok.append(int(got is not None))
    return _frozen(_bytes(memos, 5), _bytes(notes, 2), np.array(ok, dtype=np.uint32))


def run_seal(ctx, reqs_arr):
    n = reqs_arr.shape[0]
    memos, notes, ok = ctx.note_seal_view(ctx.to_device(reqs_arr))
    assert isinstance(ok, np.ndarray) and ok.dtype == np.uint32 and ok.shape == (n,)
    return _host(ctx, memos, n, 5, 32), _host(ctx, notes, n, 2, 32), ok


def case_seal(ctx):
    """memos and notes byte for byte; every refusal on its own (asserted on the spec first); with PV = PS = pk the request is the owned
    form's, E is the same and nothing else is"""
    tags, reqs, refused = zip(*seal_requests())
    want_memo, want_note, want_ok = _seal_expect(reqs)
    assert want_ok.tolist() == [int(not r) for r in refused], [t for t, r, k in zip(tags, refused, want_ok) if int(not r) != k]
    memo, note, ok = run_seal(ctx, _bytes(reqs, 7))
    _same(ok, want_ok, "seal_view ok")
    _same(memo, want_memo, "seal_view memos")
    _same(note, want_note, "seal_view notes")
    k = tags.index("PV = PS")
    with mock.patch.object(owned_note_spec, "mul", _mul):
        o_memo, o_note = owned_note_spec.seal_owned(reqs[k][0], reqs[k][1:3], *reqs[k][5:])
    assert _ints(memo[k, :2]) == list(o_memo[:2]), "E differs between the forms"
    assert not set(_ints(memo[k, 2:])) & set(o_memo[2:]) and not set(_ints(note[k])) & set(o_note)


def case_small_p_is_refused_by_the_spec():
    """no request reaches small(P): PS would be a fixed point of a hash of PV's.  With a KDF that answers t = l - sk for the spend key of
    sk, P = PS + t BASE is the identity: refused by the seal and hit 2 in the scan; with t + 1 it is BASE: sealed and opened"""
    (v, pv), (sk, ps) = view_keys()[1], spend_keys()[0]
    for t, refused in ((ELL - sk % ELL, True), (ELL - sk % ELL + 1, False)):
        with _spec_memo(), mock.patch.object(spec, "kdf", lambda s, t=t: (1, t, 2, 3)):
            got = spec.seal_view(5, pv, ps, 7, 9)
            scanned = spec.scan_view(v, ps, (*_mul(bj.BASE, 5), 1, 9, 12))
        assert (got is None) == refused
        if refused:
            assert scanned == (2, None)
        else:
            assert got[1][0] == spec.H(*bj.BASE) and scanned == (1, (t, 7, 9, got[1][0]))


# ---- scan ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def scan_pool():
    """POOL items (cls, memo, note): every class of memo the issue lists, for the scanner (view_keys()[0], spend_keys()[0])"""
    rnd = random.Random(0x71E5)
    keys = view_keys()
    (v, pv), others, (_vt, pv_top) = keys[0], keys[1:4], keys[4]
    (_s, ps), (_s2, ps2) = spend_keys()
    t = nc.torsion()
    out = []

    def sealed(to, spend=ps, e=None, amount=None):
        got = spec.seal_view(rnd.randrange(1, R) if e is None else e, to, spend, rnd.randrange(1 << 64) if amount is None else amount,
                             rnd.randrange(1 << 160))
        assert got is not None
        return got

    with _spec_memo(), mock.patch.object(note_spec, "mul", _mul), mock.patch.object(owned_note_spec, "mul", _mul):
        for amount in (0, TOP_AMOUNT, None, None):
            out.append(("mine", *sealed(pv, amount=amount)))
        for _v, opv in others:
            out.append(("other", *sealed(opv)))
        out.append(("v+l", *sealed(_mul(bj.BASE, v + ELL))))
        out.append(("to r-1", *sealed(pv_top)))
        for k in (5, 6, 7):
            out.append((f"to {('l-1', 'l+1', '2l+1')[k - 5]}", *sealed(keys[k][1])))
        # one view key, another spend key: the tag is the scanner's, the c is not
        out.append(("same v, other PS", *sealed(pv, spend=ps2)))
        out.append(("same v, PS + T8", *sealed(pv, spend=bj.affine_add(ps, t[1]))))
        memo, note = sealed(pv)
        out.append(("leaf replaced", memo, (note[0], (note[1] + 1) % R)))
        memo, note = sealed(pv, amount=5)
        out.append(("amount >= 2^128", memo[:3] + ((memo[3] + (1 << 128)) % R,) + memo[4:], note))
        memo, note = sealed(pv)
        mixed = bj.affine_add(memo[:2], t[1])
        out.append(("true tag on E + T8", (*mixed, *memo[2:]), note))
        for k in range(8):
            out.append((f"small E of order {nc._order(t[k])}", (*t[k], spec.kdf(_mul(t[k], v))[0], *memo[3:]), note))
        for k, name in enumerate(("E.x", "E.y", "tag", "enc_amount", "enc_token")):
            out.append((name + "=r", memo[:k] + (R,) + memo[k + 1:], note))
        out.append(("E off the curve", (memo[0], (memo[1] + 1) % R, *memo[2:]), note))
        # the other two forms' memos, sealed to PV: v is their `sk`
        out.append(("ordinary", *note_spec.seal(rnd.randrange(1, R), pv, rnd.randrange(1 << 64), rnd.randrange(1 << 160))))
        out.append(("owned", *owned_note_spec.seal_owned(rnd.randrange(1, R), pv, rnd.randrange(1 << 64), rnd.randrange(1 << 160))))
        while len(out) < POOL:
            out.append(("mine" if len(out) % 4 == 0 else "other", *sealed(keys[len(out) % 4][1])))
    assert len(out) == POOL
    return tuple(out)


@functools.lru_cache(None)
def scan_arrays():
    pool = scan_pool()
    return _frozen(_bytes([m for _, m, _ in pool], 5), _bytes([[n[1]] for _, _, n in pool], 1).reshape(POOL, 32))


@functools.lru_cache(None)
def scan_expect(v, ps, with_leaves):
    hits, opened = [], []
    with _spec_memo():
        for _cls, memo, note in scan_pool():
            h, o = spec.scan_view(v, ps, memo, note[1] if with_leaves else None)
            hits.append(h)
            opened.append(o if o else (0,) * 4)
    return _frozen(np.array(hits, dtype=np.uint32), _bytes(opened, 4))


def run_scan(ctx, v, ps, memos, leaves, opened=True):
    n = memos.shape[0]
    out, hit = ctx.note_scan_view(v, ps, ctx.to_device(memos), ctx.to_device(leaves) if leaves is not None else None, opened=opened)
    assert isinstance(hit, np.ndarray) and hit.dtype == np.uint32 and hit.shape == (n,) and (out is None) == (not opened)
    return (_host(ctx, out, n, 4, 32) if opened else None), hit


def case_scan(ctx):
    memos, leaves = scan_arrays()
    pool = scan_pool()
    keys = view_keys()
    v = keys[0][0]
    (_s, ps), (_s2, ps2) = spend_keys()
    by_class = lambda hits, cls: {int(h) for h, (c, _, _) in zip(hits, pool) if c == cls}
    want, want_open = scan_expect(v, ps, True)
    for cls, h in (("mine", {1}), ("other", {0}), ("v+l", {1}), ("to r-1", {0}), ("same v, other PS", {2}), ("same v, PS + T8", {2}),
                   ("leaf replaced", {2}), ("amount >= 2^128", {2}), ("true tag on E + T8", {0}), ("E off the curve", {0}), ("ordinary", {0}),
                   ("owned", {0})):
        assert by_class(want, cls) == h, (cls, by_class(want, cls))
    assert all(int(h) == 0 for h, (c, _, _) in zip(want, pool) if c.startswith("small E") or c.endswith("=r"))
    # without a leaf the scan cannot tell a sibling address's memo from its own: hit 1, with a c that is not the sealed one
    blind, blind_open = scan_expect(v, ps, False)
    for cls in ("leaf replaced", "same v, other PS", "same v, PS + T8"):
        assert by_class(blind, cls) == {1}, cls
    sibling = next(i for i, (c, _, _) in enumerate(pool) if c == "same v, other PS")
    assert _ints(blind_open[sibling])[3] != pool[sibling][2][0] and _ints(scan_expect(v, ps2, True)[1][sibling])[3] == pool[sibling][2][0]
    for k, cls in ((4, "to r-1"), (5, "to l-1"), (6, "to l+1"), (7, "to 2l+1")):
        assert by_class(scan_expect(keys[k][0], ps, True)[0], cls) == {1}, cls
    # the opened t is the KDF's output, not reduced, and opens the note's key with PS -- no row holds an x
    first = next(i for i, (c, _, _) in enumerate(pool) if c == "mine")
    t = _ints(want_open[first])[0]
    assert spec.H(*spec.one_time_key(ps, t)) == pool[first][2][0]
    assert any(_ints(row)[0] >= ELL for row, h in zip(want_open, want) if h == 1), "no opened t exercises t >= l"
    for key in (v, keys[1][0]) + tuple(k for k, _ in keys[4:]):
        for with_leaves in (True, False):
            want_hit, want_opened = scan_expect(key, ps, with_leaves)
            for opened in ((True, False) if key == v else (True,)):
                got_open, got_hit = run_scan(ctx, key, ps, memos, leaves if with_leaves else None, opened)
                _same(got_hit, want_hit, f"scan_view hits v={key:#x} leaves={with_leaves} opened={opened}")
                if opened:
                    _same(got_open, want_opened, f"scan_view opened v={key:#x} leaves={with_leaves}")
    # the sibling address, PS as bytes; and v + l as bytes: the same PV, another scalar, the same rows
    for key, spend in ((v, b"".join(c.to_bytes(32, "little") for c in ps2)), ((v + ELL).to_bytes(32, "little"), ps)):
        want_hit, want_opened = scan_expect(int.from_bytes(key, "little") if isinstance(key, bytes) else key,
                                            ps2 if isinstance(spend, bytes) else spend, True)
        got_open, got_hit = run_scan(ctx, key, spend, memos, leaves)
        _same(got_hit, want_hit, "scan_view hits, second address / v + l")
        _same(got_open, want_opened, "scan_view opened, second address / v + l")
    assert by_class(scan_expect(v, ps2, True)[0], "same v, other PS") == {1} and by_class(scan_expect(v, ps2, True)[0], "mine") == {2}
    assert scan_expect(v + ELL, ps, True)[1][first].tobytes() == want_open[first].tobytes()
    # all three scans answer 0 off their own form (v is the other two scans' `sk`: their memos were sealed to PV)
    d_memos, d_leaves = ctx.to_device(memos), ctx.to_device(leaves)
    for scan, own in ((ctx.note_scan, "ordinary"), (ctx.note_scan_owned, "owned")):
        _o, hit = scan(v, d_memos, d_leaves)
        assert {int(h) for h, (c, _, _) in zip(hit, pool) if c != own} == {0} and by_class(hit, own) == {1}, own


def case_scan_refusals(ctx):
    """v >= r, and a PS with a coordinate >= r, off the curve or small, are OG_ERR_INVALID naming the reason; n = 0 looks at nothing"""
    memos, leaves = scan_arrays()
    v, ps = view_keys()[0][0], spend_keys()[0][1]
    name = "og_note_scan_view_batch_d"
    for bad in (R, R + 5, (1 << 256) - 1):
        _expect_error(lambda: run_scan(ctx, bad, ps, memos[:2], leaves[:2]), name, "v is not a canonical")
    for k in (0, 1):
        for c in (R, ps[k] + R, (1 << 256) - 1):
            _expect_error(lambda: run_scan(ctx, v, ps[:k] + (c,) + ps[k + 1:], memos[:2], leaves[:2]), name, "ps is not a canonical")
    _expect_error(lambda: run_scan(ctx, v, (ps[0], (ps[1] + 1) % R), memos[:2], leaves[:2]), name, "ps is not on the curve")
    _expect_error(lambda: run_scan(ctx, v, (0, 0), memos[:2], None), name, "ps is not on the curve")
    for t in nc.torsion():
        _expect_error(lambda: run_scan(ctx, v, t, memos[:2], leaves[:2]), name, "ps is a small point")
    assert ctx.note_scan_view(R, (0, 0), ctx.to_device(memos[:0]), None)[1].shape == (0,)   # n = 0 looks at nothing
    assert run_scan(ctx, v, bj.affine_add(ps, nc.torsion()[1]), memos[:2], None)[1].shape == (2,)   # a mixed-order PS is a key like any other


# ---- unlock ----------------------------------------------------------------------------------------------------------------------
UNLOCK_T = (0, 1, ELL - 1, ELL, TOP_MULTIPLE, R - 1) + tuple(k * ELL + k for k in range(2, 7))   # (every count of subtractions of l from t)
UNLOCK_SK = (1, ELL - 1, ELL, R - 1)


@functools.lru_cache(None)
def unlock_rows(sk):
    """((tag, (t, amount, token, c), leaf, leaf given), ...) for the wallet of sk: the crafted t's with the spec's c -- sk + t wraps
    past l every number of times --, then every way not to unlock"""
    rnd = random.Random(0x0C10 ^ sk % 65521)
    out = []
    for t in UNLOCK_T:
        amount, token = rnd.choice((0, TOP_AMOUNT, rnd.randrange(1 << 64))), rnd.randrange(R)
        c = spec.H(*_mul(bj.BASE, (sk + t) % ELL))
        out.append((f"t={t:#x}", (t, amount, token, c), spec.leaf_of(c, amount, token)))
    good, leaf = out[1][1], out[1][2]
    out.append(("wrong c", good[:3] + ((good[3] + 1) % R,), leaf))
    out.append(("the c of x + 1", good[:3] + (spec.H(*_mul(bj.BASE, (sk + good[0] + 1) % ELL)),), leaf))
    for k, name in enumerate(("t", "amount", "token", "c")):
        out.append((name + "=r", good[:k] + (R,) + good[k + 1:], leaf))
    out.append(("t + r", (good[0] + R,) + good[1:], leaf))   # the same x mod r, and not a canonical field
    out.append(("amount=2^128", (good[0], 1 << 128, *good[2:]), spec.leaf_of(good[3], 1 << 128, good[2])))
    out.append(("zero row", (0, 0, 0, 0), leaf))
    out.append(("wrong leaf", good, (leaf + 1) % R))
    out.append(("a lie about the amount", (good[0], good[1] ^ 1, *good[2:]), leaf))
    out.append(("a lie about the token", (*good[:2], good[2] ^ 1, good[3]), leaf))
    return tuple(out)


@functools.lru_cache(None)
def _unlock_expect(sk, rows, leaves):
    oks, unlocked = [], []
    with _spec_memo():
        for k, row in enumerate(rows):
            ok, o = spec.unlock(sk, row, leaves[k] if leaves is not None else None)
            oks.append(ok)
            unlocked.append(o if o else (0,) * 4)
    return _frozen(np.array(oks, dtype=np.uint32), _bytes(unlocked, 4))


def run_unlock(ctx, sk, rows_arr, leaves_arr):
    n = rows_arr.shape[0]
    out, ok = ctx.note_unlock(sk, ctx.to_device(rows_arr), ctx.to_device(leaves_arr) if leaves_arr is not None else None)
    assert isinstance(ok, np.ndarray) and ok.dtype == np.uint32 and ok.shape == (n,)
    return _host(ctx, out, n, 4, 32), ok


def case_unlock(ctx):
    for sk in UNLOCK_SK:
        tags, rows, leaves = zip(*unlock_rows(sk))
        for with_leaves in (True, False):
            want_ok, want = _unlock_expect(sk, rows, leaves if with_leaves else None)
            by_tag = dict(zip(tags, want_ok.tolist()))
            assert all(by_tag[f"t={t:#x}"] == 1 for t in UNLOCK_T)
            assert not any(by_tag[t] for t in ("wrong c", "the c of x + 1", "t=r", "amount=r", "token=r", "c=r", "t + r", "amount=2^128", "zero row"))
            assert [by_tag[t] for t in ("wrong leaf", "a lie about the amount", "a lie about the token")] == [int(not with_leaves)] * 3
            got, ok = run_unlock(ctx, sk, _bytes(rows, 4), _bytes([[l] for l in leaves], 1).reshape(-1, 32) if with_leaves else None)
            _same(ok, want_ok, f"unlock ok sk={sk:#x} leaves={with_leaves}")
            _same(got, want, f"unlock rows sk={sk:#x} leaves={with_leaves}")
    # every count of reductions of t, and sk mod l + t mod l on both sides of l
    assert {t // ELL for t in UNLOCK_T} == set(range(8)) and max(sk + t for sk in UNLOCK_SK for t in UNLOCK_T) == 2 * R - 2
    assert {(sk % ELL + t % ELL) // ELL for sk in UNLOCK_SK for t in UNLOCK_T} == {0, 1}
    _expect_error(lambda: run_unlock(ctx, R, _bytes([(0,) * 4], 4), None), "og_note_unlock_batch_d", "sk is not a canonical")
    assert ctx.note_unlock(R, ctx.to_device(_bytes([], 4)), None)[1].shape == (0,)   # n = 0 looks at nothing


def case_unlock_opens_what_scan_owned_opens(ctx):
    """an owned note to pk = sk BASE has x = sk + t mod l; a view row with that t and the owned c, unlocked with sk, is byte for byte
    the row og_note_scan_owned_batch_d opens (the leaf shape is the same, so the owned leaf stands beside both)"""
    rnd = random.Random(0x0B7E)
    reqs = []
    for sk, pk in oc.scan_keys()[:3] + oc.scan_keys()[5:]:
        reqs.append((sk, (rnd.randrange(1, R), *pk, rnd.randrange(1 << 64), rnd.randrange(1 << 160))))
    memos_d, notes_d, ok = ctx.note_seal_owned(ctx.to_device(_bytes([r for _, r in reqs], 5)))
    assert ok.all()
    notes = _host(ctx, notes_d, len(reqs), 2, 32)
    memos = _host(ctx, memos_d, len(reqs), 5, 32)
    for k, (sk, (e, px, py, amount, token)) in enumerate(reqs):
        leaf_d = ctx.to_device(np.ascontiguousarray(notes[k, 1:2]))
        opened_d, hit = ctx.note_scan_owned(sk, ctx.to_device(np.ascontiguousarray(memos[k:k + 1])), leaf_d)
        assert hit.tolist() == [1]
        t = owned_note_spec.kdf(_mul((px, py), e))[1]
        row = _bytes([(t, amount, token, _ints(notes[k, 0])[0])], 4)
        got, ok = run_unlock(ctx, sk, row, np.ascontiguousarray(notes[k, 1:2]))
        assert ok.tolist() == [1]
        _same(got, _host(ctx, opened_d, 1, 4, 32), f"unlock against scan_owned, sk={sk:#x}")


def case_torsion_ps_never_unlocks(ctx):
    """PS' = sk BASE + T8 is on the curve and not small: a note to (PV, PS') seals, and the scan of (v, PS') opens it, leaf and all;
    no x has x BASE = P, so unlock refuses it with and without the leaf.  The same note to the honest PS unlocks."""
    rnd = random.Random(0x7085)
    (v, pv), (sk, ps) = view_keys()[0], spend_keys()[0]
    mixed = bj.affine_add(ps, nc.torsion()[1])
    reqs = [(rnd.randrange(1, R), *pv, *spend, 77, 99) for spend in (mixed, ps)]
    memos_d, notes_d, ok = ctx.note_seal_view(ctx.to_device(_bytes(reqs, 7)))
    assert ok.tolist() == [1, 1]
    leaves = np.ascontiguousarray(_host(ctx, notes_d, 2, 2, 32)[:, 1])
    memos = _host(ctx, memos_d, 2, 5, 32)
    for k, (spend, unlocks) in enumerate(((mixed, 0), (ps, 1))):
        opened, hit = run_scan(ctx, v, spend, np.ascontiguousarray(memos[k:k + 1]), leaves[k:k + 1])
        assert hit.tolist() == [1]
        with _spec_memo():
            assert spec.scan_view(v, spend, tuple(_ints(memos[k])), _ints(leaves[k])[0]) == (1, tuple(_ints(opened)))
        for with_leaf in (True, False):
            got, ok = run_unlock(ctx, sk, opened, leaves[k:k + 1] if with_leaf else None)
            assert ok.tolist() == [unlocks] and got.any() == bool(unlocks)
            if unlocks:
                x = _ints(got)[0]
                assert x == (sk + _ints(opened)[0]) % ELL and _ints(got)[1:] == _ints(opened)[1:]


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seal_pool():
    reqs = [r for _, r, _ in seal_requests()]
    reqs = tuple(reqs[i % len(reqs)] for i in range(POOL))
    return _frozen(_bytes(reqs, 7)), _seal_expect(reqs)


@functools.lru_cache(None)
def unlock_pool():
    """what a scanning service hands back for the pool: the opened rows, zero unless the hit is 1, with the leaves beside them"""
    sk = spend_keys()[0][0]
    _hits, opened = scan_expect(view_keys()[0][0], spend_keys()[0][1], True)
    rows = tuple(tuple(_ints(r)) for r in opened)
    want_ok, want = _unlock_expect(sk, rows, tuple(n[1] for _, _, n in scan_pool()))
    assert [bool(k) for k in want_ok] == [bool(r[3]) for r in rows], "every opened row of the pool unlocks, no zero row does"
    return opened, (want, want_ok)


def case_shapes(ctx, name, sizes, reuse=()):
    """every size at two offsets, then the `reuse` sizes in turn (a larger call followed by a smaller one: the output buffer of the
    decisions is reused); a memo of the scanner's in lanes 0 and 63 of the first wave, in the last wave's first lane and the last lane"""
    v, (sk, ps) = view_keys()[0][0], spend_keys()[0]
    mine = [i for i, (c, _, _) in enumerate(scan_pool()) if c == "mine"]
    calls = [(n, off) for n in sizes for off in ((0, 17) if n else (0,))] + [(n, 11 * k + 3) for k, n in enumerate(reuse)]
    for j, (n, off) in enumerate(calls):
        idx = nc._index(n, off, mine[j % len(mine)])
        if name == "seal":
            arr, outs = seal_pool()
            got = run_seal(ctx, arr[idx])
        else:
            (memos, leaves) = scan_arrays()
            if name == "scan":
                outs = scan_expect(v, ps, True)[::-1]
                got = run_scan(ctx, v, ps, memos[idx], leaves[idx])
            else:
                rows, outs = unlock_pool()
                got = run_unlock(ctx, sk, rows[idx], leaves[idx])
            for pos in (0, 63, n - 1):
                assert n <= pos or pos < 0 or got[1][pos] == 1, f"{name} n={n}: no hit in lane {pos}"
        for k, (g, o) in enumerate(zip(got, outs)):
            _same(g, o[idx], f"{name}_view n={n} off={off} output {k}")


# ---- the view key cannot spend -------------------------------------------------------------------------------------------------------
def _tob(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _siblings(depth, leaves, index):
    levels = mimc7.tree_build(leaves + [0] * ((1 << depth) - len(leaves)))
    return [levels[l][(index >> l) ^ 1] for l in range(depth)], levels[-1][0]


def case_the_view_key_cannot_spend(ctx, depth=2, seed=15):
    """a view note is sealed and its leaf appended.  The scanner holds v, PS and the opened row t | amount | token | c; a claim record
    built from all of it -- its best x' is t mod l, the only scalar it holds that has to do with P -- publishes a root that is not the
    tree's.  The wallet's record after unlock publishes the tree's root and the nullifier hash H(x, 1), which the scanner cannot name."""
    from owshen_amd import api, circuit
    from tests import claim_spec
    rnd = random.Random(seed)
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))
    v, sk = rnd.randrange(1, R), rnd.randrange(1, R)
    pv, ps = bj.multiply(bj.BASE, v), bj.multiply(bj.BASE, sk)
    amount, token = 12, rnd.randrange(1 << 160)
    memos_d, notes_d, ok = ctx.note_seal_view(ctx.to_device(_tob([rnd.randrange(1, R), *pv, *ps, amount, token]).reshape(1, 7, 32)))
    assert ok.tolist() == [1]
    c, leaf = toi(notes_d)
    leaves = [rnd.randrange(R), leaf]
    _frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(_tob(leaves)))
    sib, root_py = _siblings(depth, leaves, 1)
    assert toi(root) == [root_py]
    # everything the scanner holds
    leaf_d = ctx.to_device(_tob([leaf]))
    opened_d, hit = ctx.note_scan_view(v, ps, memos_d, leaf_d)
    assert hit.tolist() == [1]
    t, got_amount, got_token, got_c = toi(opened_d)
    p = spec.one_time_key(ps, t)
    assert (got_amount, got_token, got_c) == (amount, token, c) and mimc7.hash2(*p) == c, "the scanner can compute P and c"
    unlocked_d, ok = ctx.note_unlock(sk, opened_d, leaf_d)
    assert ok.tolist() == [1]
    x = toi(unlocked_d)[0]
    assert x == (sk + t) % ELL and toi(unlocked_d)[1:] == [amount, token, c]
    common = dict(amount=amount, index=1, siblings=sib, token=token, chain_id=1, out_commitment=rnd.randrange(R))
    thief, wallet = dict(common, x=t % ELL), dict(common, x=x)
    assert bj.multiply(bj.BASE, thief["x"]) != p and bj.multiply(bj.BASE, x) == p
    wit = ctx.to_host(circuit.claim_witness(ctx, depth, ctx.to_device(np.stack([circuit.pack_claim_inputs(**thief), circuit.pack_claim_inputs(**wallet)]))))
    pub_thief, pub_wallet = api.bytes_to_ints(wit[0, 1:5]), api.bytes_to_ints(wit[1, 1:5])
    assert pub_thief[0] != root_py, "the scanner's record publishes the tree's root"
    assert pub_wallet[0] == root_py and pub_wallet[1] == mimc7.hash2(x, 1) != pub_thief[1]
    assert pub_thief == claim_spec.build(depth, **thief)[3][1:5] and pub_wallet == claim_spec.build(depth, **wallet)[3][1:5]


# ---- through the pool --------------------------------------------------------------------------------------------------------------
def case_through_the_pool(ctx, depth=2, seed=16):
    """[v, sk] -> og_eddsa_pubkey_batch_d -> seal_view -> og_mimc7_append_d -> scan_view (a second view key gets 0) -> unlock -> claim ->
    og_verify -> the ledger appends out_leaf -> `withdraw` of the out note verifies under the new root"""
    from owshen_amd import api, circuit, groth16 as g16
    from oracle.py import withdraw as withdraw_spec
    from tests.claim_cases import _key
    from tests.transfer_cases import _key as _other_key
    rnd = random.Random(seed)
    lib = ctx._lib
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))
    v, sk, v_other = rnd.randrange(1, R), rnd.randrange(1, R), rnd.randrange(1, R)
    addr_d, _c, ok = ctx.eddsa_pubkey(ctx.to_device(_tob([v, sk])), compressed=False)
    assert ok.tolist() == [1, 1]
    addr = toi(addr_d)
    ps = tuple(addr[2:])
    token, chain_id, amount = rnd.randrange(1 << 160), 1387, 9
    memos_d, notes_d, ok = ctx.note_seal_view(ctx.to_device(_tob([rnd.randrange(1, R), *addr, amount, token]).reshape(1, 7, 32)))
    assert ok.tolist() == [1]
    c, leaf = toi(notes_d)
    leaves = [rnd.randrange(R), leaf]
    frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(_tob(leaves)))
    sib, root_py = _siblings(depth, leaves, 1)
    assert toi(root) == [root_py]
    leaf_d = ctx.to_device(_tob([leaf]))
    # the scanning service, then the wallet
    assert ctx.note_scan_view(v_other, ps, memos_d, leaf_d)[1].tolist() == [0]
    opened_d, hit = ctx.note_scan_view(v, ps, memos_d, leaf_d)
    assert hit.tolist() == [1]
    assert spec.scan_view(v, ps, tuple(toi(memos_d)), leaf) == (1, tuple(toi(opened_d)))
    unlocked_d, ok = ctx.note_unlock(sk, opened_d, leaf_d)
    assert ok.tolist() == [1]
    x, got_amount, got_token, got_c = toi(unlocked_d)
    assert (got_amount, got_token, got_c) == (amount, token, c)
    assert spec.unlock(sk, tuple(toi(opened_d)), leaf) == (1, (x, amount, token, c))
    # the claim: the whole note into an ordinary one only the claimant opens
    out = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R))
    rec = dict(x=x, amount=amount, index=1, siblings=sib, token=token, chain_id=chain_id, out_commitment=mimc7.hash2(out["nullifier"], out["secret"]))
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    _b, vk, pk_c, close = _key(ctx, depth)
    proof, pub = circuit.claim_prove(ctx, pk_c, depth, ctx.to_device(circuit.pack_claim_inputs(**rec)[None]), rs, return_public=True)
    c_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), c_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert c_pub[0] == root_py and c_pub[1] == mimc7.hash2(x, 1) and c_pub[2] == chain_id
    assert c_pub[3] == withdraw_spec.leaf_of(out["nullifier"], out["secret"], amount, token)
    # the ledger appends out_leaf; the claimant withdraws the out note
    frontier, root = ctx.mimc7_append(depth, frontier, len(leaves), ctx.to_device(np.ascontiguousarray(pub[0, 3:4])))
    leaves.append(c_pub[3])
    sib_out, root_py = _siblings(depth, leaves, 2)
    assert toi(root) == [root_py]
    _b, vk, pk_w, close = _other_key(ctx, depth, "withdraw")
    wrec = circuit.pack_inputs(out["nullifier"], out["secret"], amount, 9, 0, 2, sib_out, token=token, chain_id=chain_id)
    proof, pub = circuit.prove_from_inputs(ctx, pk_w, depth, ctx.to_device(wrec[None]), rs, return_public=True)
    w_pub = api.bytes_to_ints(pub[0])
    assert w_pub[0] == root_py and w_pub[3] == amount
    assert g16.verify(g16.vk_to_bytes(vk), w_pub, proof[0].tobytes(), lib=lib) is True
    close()
