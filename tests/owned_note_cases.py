"""Owned notes on the device -- og_note_seal_owned_batch_d and og_note_scan_owned_batch_d -- against tests/owned_note_spec.py (plain
Python over oracle/py/babyjubjub.py and oracle/py/mimc7.py); shared by the CPU-interpreter run (tests/test_emu_owned_notes.py) and the
GPU run (tests/test_gpu_owned_notes.py).  The edge inputs are those of the ordinary pair (tests/note_cases.py: small and off-curve
points, non-canonical fields, amount >= 2^128, a replaced leaf), with what the owned form adds: scanning keys at and above l, so that
the reduction of sk is exercised, a key with a torsion component, and the two forms' memos in one pool.

Layouts (include/owshen_gpu.h): seal request = e | pk.x | pk.y | amount | token; memo = E.x | E.y | tag | amount + pad_a | token + pad_t;
note = c | leaf; opened note = x | amount | token | c.  Every expected value is computed once per session from the spec and handed out
read-only.

small(P) is refused by the seal (the spec's last refusal).  No request reaches it: P = pk + H(k, 7) BASE is small only if pk is a
fixed point of a hash of itself, so the refusal is checked on the spec alone, with the KDF replaced (case_small_p_is_refused_by_the_spec)."""
import functools
import random
from unittest import mock

import numpy as np

from oracle.py import babyjubjub as bj
from oracle.py.fields import R
from tests import note_cases as nc
from tests import note_spec
from tests import owned_note_spec as spec
from tests.eddsa_keys_cases import POOL, _bytes, _host, _same

ELL = spec.ELL
_mul = nc._mul
_frozen = nc._frozen
TOP_AMOUNT = nc.TOP_AMOUNT


def _spec_memo():
    return mock.patch.object(spec, "mul", _mul)


@functools.lru_cache(None)
def scan_keys():
    """(sk, pk): the ordinary cases' keys -- the scanning key first, three others, r - 1 -- then sk = l - 1, l + 1 and 2 l + 1: both
    sides of the reduction's first and second subtraction (sk = l itself has the identity for a key, which no seal accepts)"""
    keys = nc.scan_keys() + tuple((k, _mul(bj.BASE, k)) for k in (ELL - 1, ELL + 1, 2 * ELL + 1))
    assert keys[0][0] >= ELL and keys[4][0] == R - 1 >= 7 * ELL, "the scanning keys do not exercise the reduction"
    return keys


# ---- seal ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _seal_expect(reqs):
    memos, notes, ok = [], [], []
    with _spec_memo():
        for e, px, py, amount, token in reqs:
            got = spec.seal_owned(e, (px, py), amount, token)
            memos.append(got[0] if got else (0,) * 5)
            notes.append(got[1] if got else (0,) * 2)
            ok.append(int(got is not None))
    return _frozen(_bytes(memos, 5), _bytes(notes, 2), np.array(ok, dtype=np.uint32))


def run_seal(ctx, reqs_arr):
    n = reqs_arr.shape[0]
    memos, notes, ok = ctx.note_seal_owned(ctx.to_device(reqs_arr))
    assert isinstance(ok, np.ndarray) and ok.dtype == np.uint32 and ok.shape == (n,)
    return _host(ctx, memos, n, 5, 32), _host(ctx, notes, n, 2, 32), ok


def case_seal(ctx):
    """the ordinary seal's requests: the same refusals (asserted), memos and notes of the owned form byte for byte; an owned memo is
    never an ordinary one's bytes"""
    tags, reqs, refused = zip(*nc.seal_requests())
    want_memo, want_note, want_ok = _seal_expect(reqs)
    assert want_ok.tolist() == [int(not r) for r in refused], [t for t, r, k in zip(tags, refused, want_ok) if int(not r) != k]
    memo, note, ok = run_seal(ctx, _bytes(reqs, 5))
    _same(ok, want_ok, "seal_owned ok")
    _same(memo, want_memo, "seal_owned memos")
    _same(note, want_note, "seal_owned notes")
    plain_memo, plain_note, _ok = nc._seal_expect(reqs)
    for k, r in enumerate(refused):
        if not r:
            assert memo[k, :2].tobytes() == plain_memo[k, :2].tobytes(), "E differs between the forms"
            assert memo[k, 2:].tobytes() != plain_memo[k, 2:].tobytes() and note[k].tobytes() != plain_note[k].tobytes()


def case_small_p_is_refused_by_the_spec():
    """with a KDF that answers t = l - sk for the key of sk, P = pk + t BASE is the identity: refused; with t + 1 it is BASE: sealed"""
    sk, pk = nc.scan_keys()[1]
    for t, refused in ((ELL - sk % ELL, True), (ELL - sk % ELL + 1, False)):
        with _spec_memo(), mock.patch.object(spec, "kdf", lambda s, t=t: (1, t, 2, 3)):
            got = spec.seal_owned(5, pk, 7, 9)
        assert (got is None) == refused
        if not refused:
            assert got[1][0] == spec.H(*bj.BASE)


# ---- scan ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def scan_pool():
    """POOL items (cls, memo, note): the classes of the ordinary pool in the owned form, and beside them a key with a torsion component
    and ordinary memos to the same keys"""
    rnd = random.Random(0x0E5CA2)
    keys = scan_keys()
    (sk, pk), others, (sk_top, pk_top) = keys[0], keys[1:4], keys[4]
    t = nc.torsion()
    out = []

    def sealed(to, e=None, amount=None):
        got = spec.seal_owned(rnd.randrange(1, R) if e is None else e, to, rnd.randrange(1 << 64) if amount is None else amount, rnd.randrange(1 << 160))
        assert got is not None
        return got

    with _spec_memo(), mock.patch.object(note_spec, "mul", _mul):
        for amount in (0, TOP_AMOUNT, None, None):
            out.append(("mine", *sealed(pk, amount=amount)))
        for _sk, opk in others:
            out.append(("other", *sealed(opk)))
        out.append(("sk+l", *sealed(_mul(bj.BASE, sk + ELL))))
        out.append(("to r-1", *sealed(pk_top)))
        for k in (5, 6, 7):
            out.append((f"to {('l-1', 'l+1', '2l+1')[k - 5]}", *sealed(keys[k][1])))
        memo, note = sealed(pk)
        out.append(("leaf replaced", memo, (note[0], (note[1] + 1) % R)))
        memo, note = sealed(pk, amount=5)
        out.append(("amount >= 2^128", memo[:3] + ((memo[3] + (1 << 128)) % R,) + memo[4:], note))
        # a key with a torsion component: with e a multiple of 8 the shared point is the honest key's (e T8 = O), the tag matches, and
        # c = H(x BASE) is not the sealed c = H(P) -- the note can never be claimed; with an odd e the wallet does not even see it
        mixed_pk = bj.affine_add(pk, t[1])
        out.append(("pk + T8, e = 0 mod 8", *sealed(mixed_pk, e=8 * rnd.randrange(1, R // 8))))
        out.append(("pk + T8, e odd", *sealed(mixed_pk, e=rnd.randrange(1, R) | 1)))
        memo, note = sealed(pk)
        mixed = bj.affine_add(memo[:2], t[1])
        out.append(("true tag on E + T8", (*mixed, *memo[2:]), note))
        for k in range(8):
            out.append((f"small E of order {nc._order(t[k])}", (*t[k], spec.kdf(_mul(t[k], sk))[0], *memo[3:]), note))
        for k, name in enumerate(("E.x", "E.y", "tag", "enc_amount", "enc_token")):
            out.append((name + "=r", memo[:k] + (R,) + memo[k + 1:], note))
        out.append(("E off the curve", (memo[0], (memo[1] + 1) % R, *memo[2:]), note))
        for _ in range(2):   # the other form's memo to the scanning key
            out.append(("ordinary", *note_spec.seal(rnd.randrange(1, R), pk, rnd.randrange(1 << 64), rnd.randrange(1 << 160))))
        while len(out) < POOL:
            out.append(("mine" if len(out) % 4 == 0 else "other", *sealed(keys[len(out) % 4][1])))
    assert len(out) == POOL
    return tuple(out)


@functools.lru_cache(None)
def scan_arrays():
    pool = scan_pool()
    return _frozen(_bytes([m for _, m, _ in pool], 5), _bytes([[n[1]] for _, _, n in pool], 1).reshape(POOL, 32))


@functools.lru_cache(None)
def scan_expect(sk, with_leaves):
    hits, opened = [], []
    with _spec_memo():
        for _cls, memo, note in scan_pool():
            h, o = spec.scan_owned(sk, memo, note[1] if with_leaves else None)
            hits.append(h)
            opened.append(o if o else (0,) * 4)
    return _frozen(np.array(hits, dtype=np.uint32), _bytes(opened, 4))


def run_scan(ctx, sk, memos, leaves, opened=True):
    n = memos.shape[0]
    out, hit = ctx.note_scan_owned(sk, ctx.to_device(memos), ctx.to_device(leaves) if leaves is not None else None, opened=opened)
    assert isinstance(hit, np.ndarray) and hit.dtype == np.uint32 and hit.shape == (n,) and (out is None) == (not opened)
    return (_host(ctx, out, n, 4, 32) if opened else None), hit


def case_scan(ctx):
    memos, leaves = scan_arrays()
    pool = scan_pool()
    keys = scan_keys()
    sk = keys[0][0]
    by_class = lambda hits, cls: {int(h) for h, (c, _, _) in zip(hits, pool) if c == cls}
    want, want_open = scan_expect(sk, True)
    for cls, h in (("mine", {1}), ("other", {0}), ("sk+l", {1}), ("to r-1", {0}), ("leaf replaced", {2}), ("amount >= 2^128", {2}),
                   ("pk + T8, e = 0 mod 8", {2}), ("pk + T8, e odd", {0}), ("true tag on E + T8", {0}), ("E off the curve", {0}),
                   ("ordinary", {0})):
        assert by_class(want, cls) == h, (cls, by_class(want, cls))
    assert all(int(h) == 0 for h, (c, _, _) in zip(want, pool) if c.startswith("small E") or c.endswith("=r"))
    assert by_class(scan_expect(sk, False)[0], "leaf replaced") == {1} and by_class(scan_expect(sk, False)[0], "pk + T8, e = 0 mod 8") == {1}
    for k, cls in ((4, "to r-1"), (5, "to l-1"), (6, "to l+1"), (7, "to 2l+1")):
        assert by_class(scan_expect(keys[k][0], True)[0], cls) == {1}, cls
    # the opened x is canonical mod l and opens the note's key
    first = next(i for i, (c, _, _) in enumerate(pool) if c == "mine")
    x = int.from_bytes(want_open[first, 0].tobytes(), "little")
    assert x < ELL and spec.H(*_mul(bj.BASE, x)) == pool[first][2][0]
    for key in (sk, keys[1][0]) + tuple(k for k, _ in keys[4:]):
        for with_leaves in (True, False):
            want_hit, want_opened = scan_expect(key, with_leaves)
            for opened in ((True, False) if key == sk else (True,)):
                got_open, got_hit = run_scan(ctx, key, memos, leaves if with_leaves else None, opened)
                _same(got_hit, want_hit, f"scan_owned hits sk={key:#x} leaves={with_leaves} opened={opened}")
                if opened:
                    _same(got_open, want_opened, f"scan_owned opened sk={key:#x} leaves={with_leaves}")
    # sk + l: the same public key, another scalar, the same x
    want_hit, want_opened = scan_expect(sk + ELL, True)
    got_open, got_hit = run_scan(ctx, (sk + ELL).to_bytes(32, "little"), memos, leaves)
    _same(got_hit, want_hit, "scan_owned hits sk + l")
    _same(got_open, want_opened, "scan_owned opened sk + l")
    assert by_class(want_hit, "mine") == {1} and want_opened[first].tobytes() == want_open[first].tobytes()
    # the ordinary scan answers 0 on every owned memo of the pool (and opens the ordinary ones)
    _o, plain_hit = ctx.note_scan(sk, ctx.to_device(memos), ctx.to_device(leaves))
    assert {int(h) for h, (c, _, _) in zip(plain_hit, pool) if c != "ordinary"} == {0} and by_class(plain_hit, "ordinary") == {1}


def case_scan_refuses_a_non_canonical_sk(ctx):
    from owshen_amd.api import OwshenGpuError
    memos, leaves = scan_arrays()
    for bad in (R, R + 5, (1 << 256) - 1):
        try:
            run_scan(ctx, bad, memos[:2], leaves[:2])
        except OwshenGpuError as e:
            assert e.code == -1 and "og_note_scan_owned_batch_d: sk is not a canonical" in str(e), e
        else:
            raise AssertionError(f"sk = {bad:#x} was accepted")
    assert ctx.note_scan_owned(R, ctx.to_device(memos[:0]), None)[1].shape == (0,)   # n = 0 looks at nothing


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seal_pool():
    reqs = [r for _, r, _ in nc.seal_requests()]
    reqs = tuple(reqs[i % len(reqs)] for i in range(POOL))
    return _frozen(_bytes(reqs, 5)), _seal_expect(reqs)


def case_shapes(ctx, name, sizes, reuse=()):
    """every size at two offsets, then the `reuse` sizes in turn (a larger call followed by a smaller one: the output buffer of the
    decisions is reused)"""
    sk = scan_keys()[0][0]
    mine = [i for i, (c, _, _) in enumerate(scan_pool()) if c == "mine"]
    calls = [(n, off) for n in sizes for off in ((0, 17) if n else (0,))] + [(n, 11 * k + 3) for k, n in enumerate(reuse)]
    for j, (n, off) in enumerate(calls):
        idx = nc._index(n, off, mine[j % len(mine)])
        if name == "seal":
            arr, outs = seal_pool()
            got = run_seal(ctx, arr[idx])
        else:
            (memos, leaves), outs = scan_arrays(), scan_expect(sk, True)
            outs = (outs[1], outs[0])
            got = run_scan(ctx, sk, memos[idx], leaves[idx])
            for pos in (0, 63, n - 1):
                assert n <= pos or pos < 0 or got[1][pos] == 1, f"scan_owned n={n}: no hit in lane {pos}"
        for k, (g, o) in enumerate(zip(got, outs)):
            _same(g, o[idx], f"{name}_owned n={n} off={off} output {k}")
