"""Stealth notes on the device -- og_note_seal_batch_d, og_note_scan_batch_d and the uniform-scalar seam og_hook_ed_mul_uniform_d --
against tests/note_spec.py (plain Python over oracle/py/babyjubjub.py and oracle/py/mimc7.py); shared by the CPU-interpreter run
(tests/test_emu_notes.py) and the GPU run (tests/test_gpu_notes.py).

Layouts (include/owshen_gpu.h): seal request = e | pk.x | pk.y | amount | token; memo = E.x | E.y | tag | amount + pad_a | token + pad_t;
note = c' | leaf; opened note = nullifier' | secret' | amount | token.  Every expected value is computed once per session from the spec
and handed out read-only.

The device recodes the scan's scalar as a width-4 NAF (digits 0, +-1, +-3, +-5, +-7, a carry out of every digit that comes out
negative); `seam_scalars` holds the edges of that recoding by construction."""
import ctypes as C
import functools
import random
from unittest import mock

import numpy as np

from oracle.py import babyjubjub as bj
from oracle.py import mimc7
from oracle.py.fields import R
from tests import note_spec as spec
from tests.eddsa_keys_cases import POOL, _bytes, _host, _ints, _same, _tiled_index

ELL = spec.ELL
IDENT = spec.IDENTITY
_mul = functools.lru_cache(None)(bj.multiply)   # the oracle's own multiply, memoised: points and keys repeat


def _spec_memo():
    return mock.patch.object(spec, "mul", _mul)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _point(x):
    """the curve point with this x and the even y, or None"""
    try:
        return bj.decompress((x, False))
    except ValueError:
        return None


def _order(t):
    return next(o for o in (1, 2, 4, 8) if _mul(t, o) == IDENT)


@functools.lru_cache(None)
def torsion():
    """the eight points with 8 P = (0, 1), each obtained as l Q for an on-curve Q with x in 2 .. 400; index k holds k T8"""
    found = {}
    for x in range(2, 401):
        q = _point(x)
        if q is None:
            continue
        assert bj.is_on_curve(q)
        for p in (q, (q[0], (-q[1]) % R), ((-q[0]) % R, q[1])):
            found.setdefault(_mul(p, ELL), p)
        if len(found) == 8:
            break
    assert len(found) == 8 and {_order(t) for t in found} == {1, 2, 4, 8}, sorted(_order(t) for t in found)
    t8 = next(t for t in found if _order(t) == 8)
    pts = tuple(_mul(t8, k) for k in range(8))
    assert set(pts) == set(found) and pts[0] == IDENT and all(spec.small(t) for t in pts)
    return pts


def _random_point(rnd):
    while True:
        p = _point(rnd.randrange(R))
        if p is not None:
            return p if rnd.random() < 0.5 else (p[0], (-p[1]) % R)


# ---- 1. the uniform-scalar seam --------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seam_scalars():
    rnd = random.Random(0x5CA1)
    all_max = 7 * (16 ** 63 - 1) // 15                  # 0x777...7: every digit +7, no carry anywhere
    all_carry = 16 ** 63 - all_max                      # 0x888...89: every digit -7, each carrying into the next; the top digit (+1 at
    #                                                     2^252) is made by the last carry alone
    top_by_carry = 3 * 2 ** 252 - 1                     # 0x2ff...f: -1, then a carry through 252 ones into the top digit 3
    named = [0, 1, 2, 7, 8, 15, 16, ELL - 1, ELL, ELL + 1, bj.ORDER - R, 7 * ELL, R - 1, 1 << 253, (1 << 253) - 1, all_max, all_carry,
             top_by_carry]
    assert all(0 <= s < R for s in named) and 0 < bj.ORDER - R < ELL
    assert all_max == int("7" * 63, 16) and all_carry == int("8" * 62 + "9", 16) and top_by_carry == int("2" + "f" * 63, 16)
    return tuple(named + [rnd.randrange(R) for _ in range(16)])


@functools.lru_cache(None)
def seam_points():
    rnd = random.Random(0x9017)
    t8 = torsion()[1]
    mixed = bj.affine_add(bj.BASE, t8)
    assert bj.is_on_curve(mixed) and not spec.small(mixed) and _mul(mixed, ELL) == _mul(t8, ELL % 8) != IDENT
    pts = [bj.BASE, IDENT, *torsion(), mixed] + [_random_point(rnd) for _ in range(16)]
    assert all(bj.is_on_curve(p) for p in pts)
    return tuple(pts)


def run_mul_uniform(ctx, scalar, pts):
    fn = ctx._lib.og_hook_ed_mul_uniform_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    n = len(pts)
    out, ok = ctx.empty(n, 64), np.zeros(n, dtype=np.uint32)
    d = ctx.to_device(_bytes(pts, 2))
    ctx._pre()
    skb = (C.c_uint8 * 32).from_buffer_copy(int(scalar).to_bytes(32, "little"))
    ctx._check(fn(ctx._h, skb, ctx.ptr(d), n, ctx.ptr(out), ok.ctypes.data_as(C.c_void_p)))
    got = _ints(_host(ctx, out, n, 64))
    return [(got[2 * i], got[2 * i + 1]) for i in range(n)], ok


def case_mul_uniform(ctx):
    pts = seam_points()
    off = (pts[-1][0], (pts[-1][1] + 1) % R)
    assert not bj.is_on_curve(off)
    for s in seam_scalars():
        got, ok = run_mul_uniform(ctx, s, pts + (off,))
        want = [_mul(p, s) for p in pts]
        assert ok.tolist() == [1] * len(pts) + [0] and got[-1] == (0, 0), f"ok for s = {s:#x}"
        bad = [i for i in range(len(pts)) if got[i] != want[i]]
        assert not bad, f"s = {s:#x}: points {bad[:8]} differ from multiply"
    # a non-canonical coordinate is refused like an off-curve point
    got, ok = run_mul_uniform(ctx, 5, [(bj.BASE[0] + R, bj.BASE[1]), bj.BASE])
    assert ok.tolist() == [0, 1] and got == [(0, 0), _mul(bj.BASE, 5)]


# ---- 2. seal ---------------------------------------------------------------------------------------------------------------------
TOP_AMOUNT = (1 << 128) - 1


@functools.lru_cache(None)
def scan_keys():
    """(sk, pk): the scanning key first (sk + l is a field element too), three others, then the keys of sk = r - 1"""
    rnd = random.Random(0x5EA1)
    sk = rnd.randrange(1, R - ELL) | 1    # odd: sk T8 is not the identity, whatever else
    sks = [sk] + [rnd.randrange(1, R) for _ in range(3)] + [R - 1]
    return tuple((k, _mul(bj.BASE, k)) for k in sks)


@functools.lru_cache(None)
def seal_requests():
    """((tag, (e, pk.x, pk.y, amount, token), refused), ...)"""
    rnd = random.Random(0x5EA2)
    keys = scan_keys()
    pk = keys[0][1]
    good = (rnd.randrange(1, R), pk[0], pk[1], rnd.randrange(1 << 64), rnd.randrange(1 << 160))
    out = [("random", (rnd.randrange(1, R), *keys[i % 4][1], rnd.randrange(1 << 100), rnd.randrange(R)), False) for i in range(8)]
    out += [("e=r-1", (R - 1, *good[1:]), False), ("amount=0", (*good[:3], 0, good[4]), False),
            ("amount=2^128-1", (*good[:3], TOP_AMOUNT, good[4]), False), ("token=r-1", (*good[:4], R - 1), False)]
    for k, name in enumerate(("e", "pk.x", "pk.y", "amount", "token")):
        out.append((name + "=r", good[:k] + (R,) + good[k + 1:], True))
    out.append(("all ff", good[:4] + ((1 << 256) - 1,), True))
    out.append(("amount=2^128", (*good[:3], 1 << 128, good[4]), True))
    out.append(("pk off the curve", (good[0], pk[0], (pk[1] + 1) % R, *good[3:]), True))
    for t in torsion():
        out.append((f"pk of order {_order(t)}", (good[0], *t, *good[3:]), True))
    out += [("e=0", (0, *good[1:]), True), ("e=l", (ELL, *good[1:]), True), ("e=2l", (2 * ELL, *good[1:]), True)]
    mixed = bj.affine_add(pk, torsion()[1])   # a mixed-order pk is no reason to refuse: S = e pk' like any other
    out.append(("pk + T8", (good[0], *mixed, *good[3:]), False))
    assert {_order(t) for t in torsion()} == {1, 2, 4, 8}
    return tuple(out)


@functools.lru_cache(None)
def _seal_expect(reqs):
    memos, notes, ok = [], [], []
    with _spec_memo():
        for e, px, py, amount, token in reqs:
            got = spec.seal(e, (px, py), amount, token)
            memos.append(got[0] if got else (0,) * 5)
            notes.append(got[1] if got else (0,) * 2)
            ok.append(int(got is not None))
    return _frozen(_bytes(memos, 5), _bytes(notes, 2), np.array(ok, dtype=np.uint32))


def run_seal(ctx, reqs_arr):
    n = reqs_arr.shape[0]
    memos, notes, ok = ctx.note_seal(ctx.to_device(reqs_arr))
    assert isinstance(ok, np.ndarray) and ok.dtype == np.uint32 and ok.shape == (n,)
    return _host(ctx, memos, n, 5, 32), _host(ctx, notes, n, 2, 32), ok


def case_seal(ctx):
    tags, reqs, refused = zip(*seal_requests())
    want_memo, want_note, want_ok = _seal_expect(reqs)
    assert want_ok.tolist() == [int(not r) for r in refused], [t for t, r, k in zip(tags, refused, want_ok) if int(not r) != k]
    memo, note, ok = run_seal(ctx, _bytes(reqs, 5))
    _same(ok, want_ok, "seal ok")
    _same(memo, want_memo, "seal memos")
    _same(note, want_note, "seal notes")


# ---- 3. scan ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def scan_pool():
    """POOL items (cls, memo, leaf): every class of the issue at least once -- asserted below -- filled up with memos to the four keys"""
    rnd = random.Random(0x5CA2)
    keys = scan_keys()
    (sk, pk), others, (sk_top, pk_top) = keys[0], keys[1:4], keys[4]
    t = torsion()
    out = []

    def sealed(to, e=None, amount=None):
        got = spec.seal(rnd.randrange(1, R) if e is None else e, to, rnd.randrange(1 << 64) if amount is None else amount, rnd.randrange(1 << 160))
        assert got is not None
        return got

    with _spec_memo():
        for amount in (0, TOP_AMOUNT, None, None):
            out.append(("mine", *sealed(pk, amount=amount)))
        for _sk, opk in others:
            out.append(("other", *sealed(opk)))
        alias = _mul(bj.BASE, sk + ELL)
        assert sk + ELL < R and alias == pk
        out.append(("sk+l", *sealed(alias)))
        out.append(("to r-1", *sealed(pk_top)))
        memo, note = sealed(pk)
        out.append(("leaf replaced", memo, (note[0], (note[1] + 1) % R)))
        memo, note = sealed(pk, amount=5)
        out.append(("amount >= 2^128", memo[:3] + ((memo[3] + (1 << 128)) % R,) + memo[4:], note))
        memo, note = sealed(pk)
        mixed = bj.affine_add(memo[:2], t[1])
        assert bj.is_on_curve(mixed) and not spec.small(mixed) and _mul(mixed, sk) != _mul(memo[:2], sk)
        out.append(("true tag on E + T8", (*mixed, *memo[2:]), note))
        for k in range(8):   # the tag an attacker who guessed sk T right would compute
            out.append((f"small E of order {_order(t[k])}", (*t[k], spec.kdf(_mul(t[k], sk))[0], *memo[3:]), note))
        for k, name in enumerate(("E.x", "E.y", "tag", "enc_amount", "enc_token")):
            out.append((name + "=r", memo[:k] + (R,) + memo[k + 1:], note))
        out.append(("E off the curve", (memo[0], (memo[1] + 1) % R, *memo[2:]), note))
        # what sk = 0 sees: S = (0, 1) for every E, so a memo sealed under the KDF of the identity is "its" (no pk seals to it: sk = 0
        # has the identity for a key, which `seal` refuses)
        tag, nul, sec, pad_a, pad_t = spec.kdf(IDENT)
        c = spec.H(nul, sec)
        out.append(("tag of the identity", (*memo[:2], tag, (5 + pad_a) % R, (7 + pad_t) % R), (c, spec.leaf_of(c, 5, 7))))
        while len(out) < POOL:
            out.append(("mine" if len(out) % 4 == 0 else "other", *sealed(keys[len(out) % 4][1])))
    classes = {c for c, _, _ in out}
    need = {"mine", "other", "sk+l", "to r-1", "leaf replaced", "amount >= 2^128", "true tag on E + T8", "E off the curve", "tag of the identity"}
    need |= {f"small E of order {o}" for o in (1, 2, 4, 8)} | {n + "=r" for n in ("E.x", "E.y", "tag", "enc_amount", "enc_token")}
    assert classes >= need and len(out) == POOL, need - classes
    assert sum(c.startswith("small E") for c, _, _ in out) == 8 and sum(c == "other" for c, _, _ in out) >= 3
    return tuple(out)


@functools.lru_cache(None)
def scan_arrays():
    pool = scan_pool()
    return _frozen(_bytes([m for _, m, _ in pool], 5), _bytes([[n[1]] for _, _, n in pool], 1).reshape(POOL, 32))


@functools.lru_cache(None)
def scan_expect(sk, with_leaves):
    """(hits [POOL], opened [POOL, 4, 32]) as the spec decides the pool for this key"""
    hits, opened = [], []
    with _spec_memo():
        for _cls, memo, note in scan_pool():
            h, o = spec.scan(sk, memo, note[1] if with_leaves else None)
            hits.append(h)
            opened.append(o if o else (0,) * 4)
    return _frozen(np.array(hits, dtype=np.uint32), _bytes(opened, 4))


def run_scan(ctx, sk, memos, leaves, opened=True):
    n = memos.shape[0]
    out, hit = ctx.note_scan(sk, ctx.to_device(memos), ctx.to_device(leaves) if leaves is not None else None, opened=opened)
    assert isinstance(hit, np.ndarray) and hit.dtype == np.uint32 and hit.shape == (n,) and (out is None) == (not opened)
    return (_host(ctx, out, n, 4, 32) if opened else None), hit


def case_scan(ctx):
    memos, leaves = scan_arrays()
    pool = scan_pool()
    keys = scan_keys()
    sk = keys[0][0]
    by_class = lambda hits, cls: {int(h) for h, (c, _, _) in zip(hits, pool) if c == cls}
    want, _o = scan_expect(sk, True)
    for cls, h in (("mine", {1}), ("other", {0}), ("sk+l", {1}), ("to r-1", {0}), ("leaf replaced", {2}), ("amount >= 2^128", {2}),
                   ("true tag on E + T8", {0}), ("E off the curve", {0}), ("tag of the identity", {0})):
        assert by_class(want, cls) == h, (cls, by_class(want, cls))
    assert all(int(h) == 0 for h, (c, _, _) in zip(want, pool) if c.startswith("small E") or c.endswith("=r"))
    assert by_class(scan_expect(sk, False)[0], "leaf replaced") == {1}
    assert by_class(scan_expect(0, True)[0], "tag of the identity") == {1} and by_class(scan_expect(R - 1, True)[0], "to r-1") == {1}
    for key in (sk, 0, R - 1, keys[1][0]):
        for with_leaves in (True, False):
            want_hit, want_open = scan_expect(key, with_leaves)
            for opened in (True, False):
                got_open, got_hit = run_scan(ctx, key, memos, leaves if with_leaves else None, opened)
                _same(got_hit, want_hit, f"scan hits sk={key:#x} leaves={with_leaves} opened={opened}")
                if opened:
                    _same(got_open, want_open, f"scan opened sk={key:#x} leaves={with_leaves}")
    # the key as bytes, and sk + l: the same public key, another scalar -- the spec again, on the integer
    want_hit, want_open = scan_expect(sk + ELL, True)
    got_open, got_hit = run_scan(ctx, (sk + ELL).to_bytes(32, "little"), memos, leaves)
    _same(got_hit, want_hit, "scan hits sk + l")
    _same(got_open, want_open, "scan opened sk + l")
    assert by_class(want_hit, "mine") == {1}


def case_scan_refuses_a_non_canonical_sk(ctx):
    from owshen_amd.api import OwshenGpuError
    memos, leaves = scan_arrays()
    for bad in (R, R + 5, (1 << 256) - 1):
        try:
            run_scan(ctx, bad, memos[:2], leaves[:2])
        except OwshenGpuError as e:
            assert e.code == -1 and "sk is not a canonical" in str(e), e
        else:
            raise AssertionError(f"sk = {bad:#x} was accepted")
    assert ctx.note_scan(R, ctx.to_device(memos[:0]), None)[1].shape == (0,)   # n = 0 looks at nothing


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seal_pool():
    reqs = [r for _, r, _ in seal_requests()]
    reqs = tuple(reqs[i % len(reqs)] for i in range(POOL))
    return _frozen(_bytes(reqs, 5)), _seal_expect(reqs)


def _index(n, off, hit_item):
    """the tiled pool, with a memo of the scanner's in lanes 0 and 63 of the first wave, in the first lane of the last wave and in the
    call's last lane"""
    idx = _tiled_index(n, off)
    for pos in (0, 63, (n - 1) // 64 * 64 if n else 0, n - 1):
        if 0 <= pos < n:
            idx[pos] = hit_item
    return idx


def case_shapes(ctx, name, sizes, reuse=()):
    """every size at two offsets, then the `reuse` sizes in turn (a larger call followed by a smaller one: the decisions' arena entry
    is reused)"""
    sk = scan_keys()[0][0]
    mine = [i for i, (c, _, _) in enumerate(scan_pool()) if c == "mine"]
    calls = [(n, off) for n in sizes for off in ((0, 17) if n else (0,))] + [(n, 11 * k + 3) for k, n in enumerate(reuse)]
    for j, (n, off) in enumerate(calls):
        idx = _index(n, off, mine[j % len(mine)])
        if name == "seal":
            arr, outs = seal_pool()
            got = run_seal(ctx, arr[idx])
        else:
            (memos, leaves), outs = scan_arrays(), scan_expect(sk, True)
            outs = (outs[1], outs[0])
            got = run_scan(ctx, sk, memos[idx], leaves[idx])
            for pos in (0, 63, n - 1):
                assert n <= pos or pos < 0 or got[1][pos] == 1, f"scan n={n}: no hit in lane {pos}"
        for k, (g, o) in enumerate(zip(got, outs)):
            _same(g, o[idx], f"{name} n={n} off={off} output {k}")


# ---- 5. through the pool -----------------------------------------------------------------------------------------------------------
def case_through_the_pool(ctx, depth=2, seed=8):
    """seal to a key from og_eddsa_pubkey_batch_d -> the sealed c' is the pay_commitment of a transfer, whose pay_leaf is the sealed
    leaf -> the ledger appends -> the wallet scans, opens, and spends the note by `withdraw` at the leaf's index -> og_verify accepts"""
    from owshen_amd import api, circuit, groth16 as g16
    from oracle.py import withdraw as withdraw_spec
    from tests.transfer_cases import _key, _pack
    rnd = random.Random(seed)
    lib = ctx._lib
    tob = lambda vals: np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()
    toi = lambda buf: api.bytes_to_ints(np.asarray(ctx.to_host(buf)).reshape(-1, 32))

    def siblings(leaves, index):
        levels = mimc7.tree_build(leaves + [0] * ((1 << depth) - len(leaves)))
        return [levels[l][(index >> l) ^ 1] for l in range(depth)], levels[-1][0]

    sk = rnd.randrange(1, R)
    pk_d, _c, ok = ctx.eddsa_pubkey(ctx.to_device(tob([sk])), compressed=False)
    assert ok.tolist() == [1]
    pk = tuple(toi(pk_d))
    token, chain_id, amounts = rnd.randrange(1 << 160), 1387, (3, 5, 8)
    reqs = [(rnd.randrange(1, R), *pk, a, token) for a in amounts]
    memos_d, notes_d, ok = ctx.note_seal(ctx.to_device(_bytes(reqs, 5)))
    assert ok.tolist() == [1, 1, 1]
    notes = toi(notes_d)
    commitments, sealed_leaves = notes[0::2], notes[1::2]
    # the payer spends a note of 10: 3 to the payee under the sealed c', 7 back
    note = dict(nullifier=rnd.randrange(R), secret=rnd.randrange(R), amount=10)
    leaves = [withdraw_spec.leaf_of(note["nullifier"], note["secret"], note["amount"], token)]
    frontier, root = ctx.mimc7_append(depth, ctx.to_device(np.zeros((depth, 32), dtype=np.uint8)), 0, ctx.to_device(tob(leaves)))
    sib, root_py = siblings(leaves, 0)
    assert toi(root) == [root_py]
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    t_in = dict(note, index=0, siblings=sib, token=token, chain_id=chain_id, pay_commitment=commitments[0], pay_amount=amounts[0],
                change_commitment=rnd.randrange(R))
    _b, vk, pk_t, close = _key(ctx, depth)
    proof, pub = circuit.transfer_prove(ctx, pk_t, depth, ctx.to_device(_pack(circuit, t_in)[None]), rs, return_public=True)
    t_pub = api.bytes_to_ints(pub[0])
    assert g16.verify(g16.vk_to_bytes(vk), t_pub, proof[0].tobytes(), lib=lib) is True
    close()
    assert t_pub[3] == sealed_leaves[0], "pay_leaf is not the sealed leaf"
    # the ledger appends pay_leaf, change_leaf, and the second sealed leaf (paid by somebody else); the tree is full then
    new = [t_pub[3], t_pub[4], sealed_leaves[1]]
    frontier, root = ctx.mimc7_append(depth, frontier, len(leaves), ctx.to_device(tob(new)))
    leaves += new
    sib_pay, root_py = siblings(leaves, 1)
    assert toi(root) == [root_py]
    # the wallet scans every memo of the run beside its published leaf
    opened_d, hit = ctx.note_scan(sk, memos_d, ctx.to_device(tob(sealed_leaves)))
    assert hit.tolist() == [1, 1, 1]
    opened = toi(opened_d)
    assert [opened[4 * k + 2] for k in range(3)] == list(amounts) and [opened[4 * k + 3] for k in range(3)] == [token] * 3
    nullifier, secret, amount, tok = opened[:4]
    assert mimc7.hash2(nullifier, secret) == commitments[0]
    with _spec_memo():
        assert spec.scan(sk, tuple(toi(memos_d)[:5]), sealed_leaves[0]) == (1, (nullifier, secret, amount, tok))
    # and withdraws the opened note at the leaf's index
    _b, vk, pk_w, close = _key(ctx, depth, "withdraw")
    rec = circuit.pack_inputs(nullifier, secret, amount, 9, 0, 1, sib_pay, token=tok, chain_id=chain_id)
    proof, pub = circuit.prove_from_inputs(ctx, pk_w, depth, ctx.to_device(rec[None]), rs, return_public=True)
    w_pub = api.bytes_to_ints(pub[0])
    assert w_pub[0] == root_py and w_pub[3] == amounts[0]
    assert g16.verify(g16.vk_to_bytes(vk), w_pub, proof[0].tobytes(), lib=lib) is True
    close()
