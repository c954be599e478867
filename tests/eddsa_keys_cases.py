"""BabyJubJub on the device beyond verification -- compressed keys, key derivation, batched signing -- against
oracle/py/babyjubjub.py (fr_sqrt, compress, decompress, multiply, sign_mimc7, verify_mimc7), with the textbook law of
tests/eddsa_cases.py as the second reference; shared by the CPU-interpreter run (tests/test_emu_eddsa_keys.py) and the GPU run
(tests/test_gpu_eddsa_keys.py).

Encodings (include/owshen_gpu.h): compressed key = x canonical little-endian, the parity of y in bit 255, bit 254 clear;
sign request = sk | randomness | message; verify record = pk.x | pk.y | R.x | R.y | s | message, or compressed pk | R.x | R.y | s |
message.  Every expected value below is computed once per session and handed out read-only."""
import ctypes as C
import functools
import random
from unittest import mock

import numpy as np

from oracle.py import babyjubjub as bj
from oracle.py.fields import R
from tests import eddsa_cases as ec

ELL = ec.ELL
ORDER = bj.ORDER
TOP = 1 << 255
Q_ODD = (R - 1) >> 28   # r - 1 = 2^28 q
POOL = 61               # prime: a tiled pool never lines up with the 64-lane grid


def _bytes(rows, width):
    """rows of `width` integers below 2^256 -> np.uint8 [n, width, 32]"""
    out = np.zeros((len(rows), width, 32), dtype=np.uint8)
    for i, row in enumerate(rows):
        for k, v in enumerate(row):
            out[i, k] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    return out


def _ints(arr):
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    return [int.from_bytes(a.reshape(-1, 32)[i].tobytes(), "little") for i in range(a.size // 32)]


def _host(ctx, buf, *shape):
    return np.asarray(ctx.to_host(buf)).reshape(*shape)


def encode(p):
    """the 32-byte compressed key of a point, as an integer"""
    x, odd = bj.compress(p)
    return x | (TOP if odd else 0)


def decode_expect(c):
    """(x, y) as the oracle decompresses the encoding c, or None: refused (x >= r, bit 254) or "Cannot take sqrt" """
    x, odd = c & (TOP - 1), bool(c >> 255)
    if x >= R:   # (covers bit 254: r < 2^254)
        return None
    try:
        p = bj.decompress((x, odd))
    except ValueError:
        return None
    assert ec.td_on_curve(p) and (p[1] == 0 or bool(p[1] & 1) == odd)
    return p


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.reshape(len(want), -1) != want.reshape(len(want), -1)).any(axis=1)) if len(want) else []
    assert len(bad) == 0, f"{what}: items {list(bad[:12])}{' ...' if len(bad) > 12 else ''} differ from the oracle"


# ---- 1. the square-root seam -----------------------------------------------------------------------------------------------------
def sqrt_depth(a):
    """log2 of the order of a^q in the 2^28-th roots of unity (28 for a non-residue): the level Tonelli-Shanks starts from"""
    t, k = pow(a, Q_ODD, R), 0
    while t != 1:
        t, k = t * t % R, k + 1
    return k


@functools.lru_cache(None)
def sqrt_inputs():
    rnd = random.Random(0x5157)
    vals = [0, 1, R - 1, 4]
    vals += [pow(7, (1 << k) * (rnd.randrange(1 << 60) | 1), R) for k in range(1, 29)]   # depth 28 - k: 27 .. 0
    vals += [pow(7, rnd.randrange(R) | 1, R) for _ in range(4)]                            # 7^odd: non-residues
    while sum(pow(v, (R - 1) // 2, R) == R - 1 for v in vals) < 10:                        # a few random non-residues
        v = rnd.randrange(1, R)
        if pow(v, (R - 1) // 2, R) == R - 1:
            vals.append(v)
    vals += [pow(rnd.randrange(1, R), 2, R) for _ in range(64)]
    depths = {sqrt_depth(v) for v in vals if v and pow(v, (R - 1) // 2, R) == 1}
    assert depths >= set(range(28)), sorted(set(range(28)) - depths)
    assert pow(R - 1, (R - 1) // 2, R) == 1   # r = 1 (mod 4): -1 is a residue
    return tuple(vals)


def _hook(ctx, name):
    fn = getattr(ctx._lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return fn


def run_fr_sqrt(ctx, vals):
    n = len(vals)
    out, ok = ctx.empty(n, 32), np.zeros(n, dtype=np.uint32)
    a = ctx.to_device(_bytes([[v] for v in vals], 1))
    ctx._pre()
    ctx._check(_hook(ctx, "og_hook_fr_sqrt_d")(ctx._h, ctx.ptr(a), n, ctx.ptr(out), ok.ctypes.data_as(C.c_void_p)))
    return _ints(_host(ctx, out, n, 32)), ok


def case_fr_sqrt(ctx):
    vals = sqrt_inputs()
    roots, ok = run_fr_sqrt(ctx, vals)
    for a, y, k in zip(vals, roots, ok.tolist()):
        assert k in (0, 1) and y < R
        if k:
            assert y * y % R == a, f"root^2 != a for a = {a:#x} (depth {sqrt_depth(a)})"
        else:
            assert pow(a, (R - 1) // 2, R) == R - 1 and y == 0, f"a = {a:#x} (depth {sqrt_depth(a)}) is a residue and was refused"
    assert 10 <= int(ok.sum()) <= len(vals) - 10
    # a non-canonical element is refused, whatever it reduces to
    roots, ok = run_fr_sqrt(ctx, [4 + R, (1 << 256) - 1])
    assert ok.tolist() == [0, 0] and roots == [0, 0]


# ---- 2. the mod-ORDER seam -------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sign_s_triples():
    """(r, h, sk), all below the field modulus"""
    rnd = random.Random(0x0DE8)
    out = [(0, 0, 0), (R - 1, R - 1, R - 1), (R - 1, 1, 2)]
    assert (R - 1 + 2) % ORDER == R + 1 and R + 1 < ORDER   # an s >= r exists: ORDER - r > 0

    def solve(target):   # h sk + r = target (mod ORDER), redrawn until r is a field element
        while True:
            h, sk = rnd.randrange(R), rnd.randrange(R)
            r = (target - h * sk) % ORDER
            if r < R:
                return (r, h, sk)

    out += [solve(t) for t in (0, 1, ORDER - 1, R - 1, R, ELL, ELL - 1, 7 * ELL)]
    out += [solve(rnd.randrange(ORDER) // 8 * 8 + low) for low in range(8)]   # the sum's three low bits: the second CRT residue
    out += [(rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)) for _ in range(64)]
    assert {(r + h * sk) % ORDER % 8 for r, h, sk in out} == set(range(8))
    return tuple(out)


def case_sign_s(ctx):
    tr = sign_s_triples()
    n = len(tr)
    out, ok = ctx.empty(n, 32), np.zeros(n, dtype=np.uint32)
    d = ctx.to_device(_bytes(tr, 3))
    ctx._pre()
    ctx._check(_hook(ctx, "og_hook_ed_sign_s_d")(ctx._h, ctx.ptr(d), n, ctx.ptr(out), ok.ctypes.data_as(C.c_void_p)))
    want = [(r + h * sk) % ORDER for r, h, sk in tr]
    got = _ints(_host(ctx, out, n, 32))
    bad = [i for i in range(n) if got[i] != want[i] or int(ok[i]) != int(want[i] < R)]
    assert not bad, [(i, tr[i], hex(got[i]), hex(want[i]), int(ok[i])) for i in bad[:4]]
    assert 0 in ok.tolist() and int(ok[2]) == 0


# ---- 3. decompression ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def decompress_keys():
    """((tag, encoding), ...) with every kind the issue lists"""
    rnd = random.Random(0xDEC0)
    t2, t4, t8 = ec.low_order_points(rnd)
    out = []
    keys = [ec._bj_multiply(bj.BASE, rnd.randrange(1, ELL)) for _ in range(8)]
    while len({p[1] & 1 for p in keys}) < 2:
        keys.append(ec._bj_multiply(bj.BASE, rnd.randrange(1, ELL)))
    out += [("k BASE", encode(p)) for p in keys]
    out += [("x=0", 0), ("x=0,odd", TOP)]
    assert decode_expect(0) == (0, R - 1) and decode_expect(TOP) == (0, 1)
    for x in (t4[0], R - t4[0]):   # +- 1 / sqrt a: y = 0 for either flag
        assert decode_expect(x) == (x, 0) and decode_expect(x | TOP) == (x, 0)
        out += [("y=0", x), ("y=0,odd", x | TOP)]
    for name, t in (("T2", t2), ("T4", t4), ("T8", t8)):
        p = ec.td_add(keys[len(out) % len(keys)], t)
        assert decode_expect(encode(p)) == p
        out.append(("k BASE+" + name, encode(p)))
    census = [0, 0]
    while min(census) < 8:
        c = rnd.randrange(R) | (TOP if rnd.random() < 0.5 else 0)
        census[decode_expect(c) is not None] += 1
        out.append(("random x", c))
    small = next(p for p in (ec._bj_multiply(bj.BASE, k) for k in range(1, 200)) if p[0] + R < (1 << 254))
    out += [("x+r", encode(small) + R), ("r", R), ("bit 254", encode(keys[0]) | (1 << 254)), ("all ff", (1 << 256) - 1)]
    assert all(decode_expect(c) is None for _, c in out[-4:]) and decode_expect(encode(small)) == small
    return tuple(out)


@functools.lru_cache(None)
def _decompress_expect(encs):
    pts = [decode_expect(c) for c in encs]
    want = _bytes([p if p else (0, 0) for p in pts], 2).reshape(len(encs), 64)
    ok = np.array([p is not None for p in pts], dtype=np.uint32)
    want.setflags(write=False)
    ok.setflags(write=False)
    return want, ok


def run_decompress(ctx, encs):
    n = len(encs)
    pk, ok = ctx.eddsa_decompress(ctx.to_device(_bytes([[c] for c in encs], 1).reshape(n, 32)))
    assert isinstance(ok, np.ndarray) and ok.dtype == np.uint32 and ok.shape == (n,)
    return _host(ctx, pk, n, 64), ok


def case_decompress(ctx):
    tags, encs = zip(*decompress_keys())
    want, want_ok = _decompress_expect(encs)
    got, ok = run_decompress(ctx, encs)
    _same(ok, want_ok, "decompress ok")
    _same(got, want, "decompress bytes")
    assert 8 <= int(want_ok.sum()) <= len(encs) - 8
    for c, row, k in zip(encs, got, ok.tolist()):   # compress(decompress(c)) = c
        x, y = _ints(row)
        if k and y:
            assert encode((x, y)) == c
        if k and not y:
            assert encode((x, y)) == c & (TOP - 1)


# ---- 4. key derivation -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def pubkey_sks():
    rnd = random.Random(0x9B)
    sks = [0, 1, 2, 8, ELL - 1, ELL, ELL + 1, R - 1, 123456] + [rnd.randrange(R) for _ in range(6)]
    return tuple(sks + [5 + R, sks[-1] + R, (1 << 256) - 1])


@functools.lru_cache(None)
def _pubkey_expect(sks):
    pts = [ec._bj_multiply(bj.BASE, sk) if sk < R else None for sk in sks]
    for sk, p in zip(sks, pts):
        assert p is None or p == ec.td_mul(bj.BASE, sk % ELL)   # the second reference
    pk = _bytes([p if p else (0, 0) for p in pts], 2).reshape(len(sks), 64)
    pkc = _bytes([[encode(p) if p else 0] for p in pts], 1).reshape(len(sks), 32)
    ok = np.array([p is not None for p in pts], dtype=np.uint32)
    for a in (pk, pkc, ok):
        a.setflags(write=False)
    return pk, pkc, ok


def run_pubkey(ctx, sks, affine=True, compressed=True):
    n = len(sks)
    pk, pkc, ok = ctx.eddsa_pubkey(ctx.to_device(_bytes([[s] for s in sks], 1).reshape(n, 32)), affine=affine, compressed=compressed)
    assert (pk is None) == (not affine) and (pkc is None) == (not compressed) and ok.dtype == np.uint32 and ok.shape == (n,)
    return (_host(ctx, pk, n, 64) if affine else None), (_host(ctx, pkc, n, 32) if compressed else None), ok


def case_pubkey(ctx):
    sks = pubkey_sks()
    want_pk, want_pkc, want_ok = _pubkey_expect(sks)
    assert _ints(want_pk[0]) == [0, 1] and _ints(want_pk[5]) == [0, 1] and want_ok.tolist()[-3:] == [0, 0, 0]
    for affine, compressed in ((True, True), (True, False), (False, True)):   # NULL for either output
        pk, pkc, ok = run_pubkey(ctx, sks, affine, compressed)
        _same(ok, want_ok, "pubkey ok")
        if affine:
            _same(pk, want_pk, "pubkey x | y")
        if compressed:
            _same(pkc, want_pkc, "pubkey compressed")


# ---- 5. signing ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sign_requests():
    rnd = random.Random(0x516)
    reqs = [(123456, 2345, 123456)]   # the reference's fixed inputs (babyjubjub/tests.rs:40-51)
    reqs += [(rnd.randrange(1, R), rnd.randrange(R), rnd.randrange(R)) for _ in range(6)]
    reqs += [(sk, rnd.randrange(R), rnd.randrange(R)) for sk in (0, 1, ELL, R - 1)]
    reqs += [(rnd.randrange(1, R), 0, 0), (R - 1, R - 1, R - 1)]
    good = reqs[1]
    for k in range(3):   # non-canonical fields, one at a time
        reqs += [good[:k] + (good[k] + R,) + good[k + 1:], good[:k] + ((1 << 256) - 1,) + good[k + 1:]]
    return tuple(reqs)


@functools.lru_cache(None)
def _sign_expect(reqs):
    rows, ok = [], []
    with mock.patch.object(bj, "multiply", ec._bj_multiply):   # the oracle's own multiply, memoised: keys repeat
        for sk, rand_, msg in reqs:
            try:
                if max(sk, rand_, msg) >= R:
                    raise ValueError("non-canonical")
                rr, s = bj.sign_mimc7(sk, rand_, msg)
                pk = bj.multiply(bj.BASE, sk)
                rows.append((pk[0], pk[1], rr[0], rr[1], s, msg))
                ok.append(1)
            except ValueError:
                rows.append((0,) * 6)
                ok.append(0)
    want, ok = _bytes(rows, 6), np.array(ok, dtype=np.uint32)
    want.setflags(write=False)
    ok.setflags(write=False)
    return want, ok


def run_sign(ctx, reqs):
    n = len(reqs)
    recs_d, ok = ctx.eddsa_sign(ctx.to_device(_bytes(reqs, 3)))
    assert ok.dtype == np.uint32 and ok.shape == (n,)
    return recs_d, _host(ctx, recs_d, n, 6, 32), ok


def compressed_records(recs):
    """[n, 6, 32] affine records -> [n, 5, 32]: pk replaced by its compressed form (host side: the parity bit of y into x)"""
    out = np.ascontiguousarray(recs[:, 1:, :]).copy()
    out[:, 0, :] = recs[:, 0, :]
    out[:, 0, 31] |= (recs[:, 1, 0] & 1) << 7
    return out


def case_sign(ctx):
    reqs = sign_requests()
    want, want_ok = _sign_expect(reqs)
    assert want_ok.tolist() == [1] * 13 + [0] * 6
    recs_d, got, ok = run_sign(ctx, reqs)
    _same(ok, want_ok, "sign ok")
    _same(got, want, "sign records")
    # sign -> verify with no host step: the device buffer as it is
    _same(ctx.eddsa_verify(recs_d), want_ok, "verify(sign)")
    _same(ctx.eddsa_verify_compressed(ctx.to_device(compressed_records(got))), want_ok, "verify_compressed(sign)")


# ---- 6. verification with compressed keys ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def vc_records(m=None):
    """((kind, (pkc, R.x, R.y, s, msg), expected), ...): the pool records of eddsa_cases whose key is two field elements, the key
    compressed (an off-curve key: its x with the parity of its y), then keys that do not decompress and refused encodings.
    kind: "ok", "signature" (decompresses, rejected), "sqrt", "encoding" """
    rnd = random.Random(0xC0)
    out = []
    for rec in ec.pool_records()[:m]:
        if max(rec.pk) >= R:
            continue
        c = encode(rec.pk)
        p = decode_expect(c)
        if p is None:
            out.append(("sqrt", (c, *rec.rr, rec.s, rec.msg), 0))
            continue
        if p == rec.pk:
            d = ec.decide(rec)   # both references on the affine record, computed once per session
        elif max(*rec.rr, rec.s, rec.msg) >= R:
            d = 0
        else:
            with mock.patch.object(bj, "multiply", ec._bj_multiply):
                d = int(bj.verify_mimc7(p, rec.msg, (rec.rr, rec.s)))
        out.append(("ok" if d else "signature", (c, *rec.rr, rec.s, rec.msg), d))
    honest = next(r for r in ec.pool_records() if r.cls == 8 and r.tag == "canonical")
    assert ec.decide(honest) == 1 and decode_expect(encode(honest.pk)) == honest.pk
    rest = (*honest.rr, honest.s, honest.msg)
    c = encode(honest.pk)
    out.append(("signature", (c ^ TOP, *rest), 0))   # the other root: -pk.y
    for _ in range(2):
        x = next(x for x in iter(lambda: rnd.randrange(R), None) if decode_expect(x) is None)
        out.append(("sqrt", (x, *rest), 0))
    out += [("encoding", (c | (1 << 254), *rest), 0), ("encoding", ((1 << 256) - 1, *rest), 0), ("encoding", (R, *rest), 0)]
    if (c & (TOP - 1)) + R < (1 << 254):
        out.append(("encoding", (c + R, *rest), 0))
    kinds = {k for k, _, _ in out}
    assert kinds == {"ok", "signature", "sqrt", "encoding"}, kinds
    assert all((k == "ok") == bool(d) for k, _, d in out)
    return tuple(out)


def case_verify_compressed(ctx, m=None):
    recs = vc_records(m)
    want = np.array([d for _, _, d in recs], dtype=np.uint32)
    got = ctx.eddsa_verify_compressed(ctx.to_device(_bytes([r for _, r, _ in recs], 5)))
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), recs[i][0], int(got[i]), int(want[i])) for i in bad[:12]]
    print("verify_compressed: %d records, %s" % (len(recs), {k: sum(r[0] == k for r in recs) for k in ("ok", "signature", "sqrt", "encoding")}))


# ---- 7. shapes -------------------------------------------------------------------------------------------------------------------
def _pool(items):
    """the first POOL of `items`, cycled when there are fewer (expected values repeat with them)"""
    return tuple(items[i % len(items)] for i in range(POOL))


@functools.lru_cache(None)
def shape_pools():
    """call name -> (input array [POOL, ...], tuple of expected arrays [POOL, ...]); inputs and outputs read-only"""
    encs = _pool([c for _, c in decompress_keys()])
    sks = _pool(pubkey_sks() + tuple(random.Random(0x61).randrange(R) for _ in range(POOL)))
    reqs = _pool(sign_requests())
    vc = _pool(vc_records(POOL))
    pools = {
        "decompress": (_bytes([[c] for c in encs], 1).reshape(POOL, 32), _decompress_expect(encs)),
        "pubkey": (_bytes([[s] for s in sks], 1).reshape(POOL, 32), _pubkey_expect(sks)),
        "sign": (_bytes(reqs, 3), _sign_expect(reqs)),
        "verify_compressed": (_bytes([r for _, r, _ in vc], 5), (np.array([d for _, _, d in vc], dtype=np.uint32),)),
    }
    for arr, outs in pools.values():
        arr.setflags(write=False)
        for o in outs:
            o.setflags(write=False)
    return pools


def _call(ctx, name, arr):
    n = arr.shape[0]
    d = ctx.to_device(arr)
    if name == "decompress":
        pk, ok = ctx.eddsa_decompress(d)
        return _host(ctx, pk, n, 64), ok
    if name == "pubkey":
        pk, pkc, ok = ctx.eddsa_pubkey(d)
        return _host(ctx, pk, n, 64), _host(ctx, pkc, n, 32), ok
    if name == "sign":
        recs, ok = ctx.eddsa_sign(d)
        return _host(ctx, recs, n, 6, 32), ok
    return (ctx.eddsa_verify_compressed(d),)


def _tiled_index(n, off):
    return (np.arange(n, dtype=np.int64) * 7 + n + off) % POOL


def other_offset(outs, n):
    """the first offset at which SOME expected output differs from offset 0's in the call's last lane: a lane that is never written
    keeps one value over both calls and fails one of them, whatever the buffer held"""
    last = lambda off: (7 * (n - 1) + n + off) % POOL
    return next(off for off in range(1, POOL) if any(not np.array_equal(o[last(off)], o[last(0)]) for o in outs))


def case_shapes(ctx, name, sizes, reuse=()):
    """every size twice (offset 0 and other_offset), then the `reuse` sizes in turn: the decisions' arena entry is reused across
    calls of different n"""
    arr, outs = shape_pools()[name]
    calls = [(n, off) for n in sizes for off in ((0, other_offset(outs, n)) if n else (0,))]
    calls += [(n, 11 * k + 3) for k, n in enumerate(reuse)]
    for n, off in calls:
        idx = _tiled_index(n, off)
        got = _call(ctx, name, arr[idx])
        assert len(got) == len(outs)
        for j, (g, o) in enumerate(zip(got, outs)):
            _same(g, o[idx], f"{name} n={n} off={off} output {j}")
