"""Powers-of-tau cases shared by the CPU-interpreter run (test_emu_setup_ptau.py) and the GPU run (test_gpu_setup_ptau.py):
og_ptau_info / og_setup_ptau / og_pk_contribute.  The anchor: a .ptau built HERE from a known (tau, alpha, beta) must give the
bytes og_setup(r1cs, tau, alpha, beta, gamma = 1, delta = 1) gives -- the whole proving-key blob and the whole verifying-key
blob --, and after a contribution by delta' the bytes of og_setup(.., 1, delta').  Canonical affine output makes the result
independent of the path: fixed-base multiplications by known scalars there, DFTs over points and a sparse product over points
here.  No file made by snarkjs is involved; the writer below follows the layout include/owshen_gpu.h documents."""
import random
import struct

import numpy as np
import pytest

from oracle.py import fields
from oracle.py.curve import G2_B
from tests.r1cs_util import random_r1cs

R, P = fields.R, fields.P
_CACHE = {}


# ---- the test-side writer -------------------------------------------------------------------------------------------------
def _enc(coord_bytes):
    """canonical 32-byte little-endian coordinates -> the file's: x 2^256 mod q, little-endian"""
    raw = bytes(coord_bytes)
    return b"".join(((int.from_bytes(raw[o:o + 32], "little") << 256) % P).to_bytes(32, "little") for o in range(0, len(raw), 32))


def _points(ctx, group, scalars):
    from owshen_amd import api, groth16 as g16
    base = g16.G1_GEN_BYTES if group == 1 else g16.G2_GEN_BYTES
    out = ctx.to_host(ctx.scalar_mul(group, base, ctx.to_device(api.ints_to_bytes(scalars))))
    return _enc(np.asarray(out).tobytes())


def _file(sections, magic=b"ptau", version=1):
    out = magic + struct.pack("<II", version, len(sections))
    for sid, body in sections:
        out += struct.pack("<IQ", sid, len(body)) + body
    return out


def ptau_sections(ctx, power, tau, alpha, beta):
    """the sections of a power-`power` file for (tau, alpha, beta): tau^i, alpha tau^i, beta tau^i as Python integers, the points
    by the library's fixed-base multiplication, the Montgomery encoding in Python; plus an empty section 7 and a dummy section 12"""
    key = (power, tau, alpha, beta)
    if key not in _CACHE:
        n = 1 << power
        tp = [pow(tau, i, R) for i in range(2 * n - 1)]
        g1 = _points(ctx, 1, tp + [alpha * t % R for t in tp[:n]] + [beta * t % R for t in tp[:n]])
        g2 = _points(ctx, 2, tp[:n] + [beta])
        hdr = struct.pack("<I", 32) + P.to_bytes(32, "little") + struct.pack("<II", power, power)
        _CACHE[key] = [(1, hdr), (2, g1[:(2 * n - 1) * 64]), (3, g2[:n * 128]), (4, g1[(2 * n - 1) * 64:(3 * n - 1) * 64]),
                       (5, g1[(3 * n - 1) * 64:]), (6, g2[n * 128:]), (7, b""), (12, b"\x5a" * 77)]
    return list(_CACHE[key])


def make_ptau(ctx, power, tau, alpha, beta):
    return _file(ptau_sections(ctx, power, tau, alpha, beta))


def _toxic(seed):
    rnd = random.Random(seed)
    return tuple(rnd.randrange(2, R) for _ in range(3))


def _small(n_constraints, n_pub):
    from owshen_amd import groth16 as g16
    n_wires, cons, z0 = random_r1cs(n_constraints, n_pub, seed=n_constraints + 5000)
    return g16.R1CS.from_constraints(n_wires, n_pub, cons)


def _deposit(ctx):
    from owshen_amd import circuit
    return circuit.deposit_r1cs(ctx.mimc7_constants())


def _setup_pair(ctx, r1cs, toxic, delta=1):
    """og_setup's blobs for gamma = 1"""
    from owshen_amd import groth16 as g16
    key = ("setup", id(type(ctx)), r1cs.n_wires, r1cs.n_constraints, r1cs.a.val.tobytes()[:4096], toxic, delta)
    if key not in _CACHE:
        pk, vk = g16.setup(ctx, r1cs, *toxic, 1, delta)
        _CACHE[key] = (pk, g16.vk_to_bytes(vk))
    return _CACHE[key]


def _assert_same_key(got, want):
    pk, vk = got
    want_pk, want_vk = want
    assert vk == want_vk
    assert len(pk) == len(want_pk) and pk[:592] == want_pk[:592]          # header, then alpha / beta / delta in both groups
    assert pk == want_pk


# ---- 1: equals og_setup -------------------------------------------------------------------------------------------------------
def case_equals_setup(ctx, r1cs, seed, extra_power=0):
    from owshen_amd import ptau
    toxic = _toxic(seed)
    data = make_ptau(ctx, r1cs.log_d + extra_power, *toxic)
    _assert_same_key(ptau.setup(ctx, r1cs, data), _setup_pair(ctx, r1cs, toxic))


def case_equals_setup_small(ctx, n_constraints, n_pub, extra_power=0):
    r1cs = _small(n_constraints, n_pub)
    assert r1cs.log_d == max(1, (n_constraints + n_pub).bit_length())
    case_equals_setup(ctx, r1cs, 100 + n_constraints, extra_power)


def case_equals_setup_deposit(ctx):
    r1cs = _deposit(ctx)
    assert (r1cs.n_wires, r1cs.log_d) == (735, 10)
    case_equals_setup(ctx, r1cs, 735)


# ---- 2: long and empty columns ------------------------------------------------------------------------------------------------
def long_column_r1cs():
    """350 constraints over 40 wires through og_r1cs_from_csr: wire 1 sits in every row of A, B and C with a random coefficient (a
    column of 351 terms in A -- several waves of terms, one level of 32-term runs before the final sum -- and of 1 051 terms in
    the IC / L product: 33 runs, so a SECOND level over the first level's outputs), wire 7 never occurs in B (infinity in B1 /
    B2), wire 9 occurs nowhere; coefficients 1, r - 1, small and full-width values, explicit zeros and one value above r with
    bit 255 set (og_r1cs_from_csr takes it, og_setup reduces it); some rows empty"""
    from owshen_amd import groth16 as g16
    rnd = random.Random(300)
    n_wires, n_pub, nc = 40, 2, 350
    mats = []
    for k in range(3):
        ptr, col, val = [0], [], []
        for row in range(nc):
            if not (k == 2 and row % 11 == 3):                   # (an empty row of C now and then)
                ent = {1: rnd.randrange(1, R)}
                for _ in range(rnd.randrange(0, 5)):
                    w = rnd.choice([w for w in range(n_wires) if w not in (1, 9) and not (k == 1 and w == 7)])
                    ent[w] = rnd.choice([1, R - 1, 2, rnd.randrange(R), rnd.randrange(R), 0 if row % 7 == 0 else 1])
                if k == 0 and row == 5:
                    ent[3] = (1 << 255) + 5
                for w in sorted(ent):
                    col.append(w)
                    val.append(ent[w].to_bytes(32, "little"))
            ptr.append(len(col))
        mats.append(g16.SparseMatrix(np.array(ptr, np.uint32), np.array(col, np.uint32),
                                     np.frombuffer(b"".join(val), np.uint8).reshape(-1, 32).copy(), n_wires))
    assert any(v == bytes(32) for v in [bytes(x) for x in mats[0].val])         # an explicit zero made it in
    return g16.R1CS(n_wires, n_pub, *mats)


def case_long_and_empty_columns(ctx):
    from owshen_amd import ptau
    r1cs = long_column_r1cs()
    assert r1cs.log_d == 9
    toxic = _toxic(9)
    pk, vk = ptau.setup(ctx, r1cs, make_ptau(ctx, 9, *toxic))
    _assert_same_key((pk, vk), _setup_pair(ctx, r1cs, toxic))
    m = r1cs.n_wires
    pad = lambda n: (n + 31) // 32 * 32                                                    # noqa: E731
    tail = pad(64 * m) * 2 + pad(128 * m) + pad(64 * (m - 3)) + pad(64 * 511)
    b1 = pk[len(pk) - tail + pad(64 * m):][:64 * m]
    b2 = pk[len(pk) - tail + 2 * pad(64 * m):][:128 * m]
    for w in (7, 9):
        assert b1[64 * w:64 * w + 64] == bytes(64) and b2[128 * w:128 * w + 128] == bytes(128)    # infinity
    assert b1[64:128] != bytes(64)


# ---- 3: contribute ----------------------------------------------------------------------------------------------------------------
def case_contribute(ctx, r1cs, seed):
    from owshen_amd import ptau
    from owshen_amd.api import OwshenGpuError
    toxic = _toxic(seed)
    rnd = random.Random(seed + 1)
    d1, d2 = rnd.randrange(2, R), rnd.randrange(2, R)
    pk0, vk0 = ptau.setup(ctx, r1cs, make_ptau(ctx, r1cs.log_d, *toxic))
    one = ptau.contribute(ctx, pk0, vk0, d1)
    _assert_same_key(one, _setup_pair(ctx, r1cs, toxic, d1))
    two = ptau.contribute(ctx, *one, d2)
    _assert_same_key(two, ptau.contribute(ctx, pk0, vk0, d1 * d2 % R))
    for bad in (0, R, R + 5, (1 << 256) - 1):
        with pytest.raises(OwshenGpuError) as e:
            ptau.contribute(ctx, pk0, vk0, bad)
        assert e.value.code == -1 and "og_pk_contribute" in str(e.value)
    with pytest.raises(OwshenGpuError):                     # a verifying key of another ceremony
        ptau.contribute(ctx, pk0, one[1], d1)
    return one


def case_contribute_imported(ctx):
    """a pair that came from og_zkey_import (header flag 1, n_rows = d, no C matrix): the delta step gives the import of the same
    ceremony with delta delta' in place of delta, byte for byte"""
    from oracle.py import zkey as zo
    from owshen_amd import ptau, zkey as zk
    n_wires, cons, _z0 = random_r1cs(11, 2, seed=4711)
    tau, alpha, beta, gamma, delta = (random.Random(4712).randrange(2, R) for _ in range(5))
    d1 = random.Random(4713).randrange(2, R)
    pk, vk = zk.import_zkey(ctx, zo.write_zkey(zo.snarkjs_setup(n_wires, 2, cons, tau, alpha, beta, gamma, delta)))
    assert struct.unpack("<10Q", pk[:80])[8] == 1
    want = zk.import_zkey(ctx, zo.write_zkey(zo.snarkjs_setup(n_wires, 2, cons, tau, alpha, beta, gamma, delta * d1 % R)))
    _assert_same_key(ptau.contribute(ctx, pk, vk, d1), want)


def case_contribute_small(ctx):
    case_contribute(ctx, _small(25, 3), 125)


def case_contribute_deposit(ctx):
    case_contribute(ctx, _deposit(ctx), 735)


# ---- 4: the key works -------------------------------------------------------------------------------------------------------------
def case_key_works(ctx, n=64):
    """the deposit key from a .ptau, after a contribution: n proofs through og_deposit_prove_batch_d are accepted by og_verify and by
    og_verify_batch_d, a wrong public input is refused, and the first and last proofs are the C restatement's"""
    from oracle.c import binding as oc
    from owshen_amd import circuit, groth16 as g16, ptau
    r1cs = _deposit(ctx)
    toxic = _toxic(735)
    pk0, vk0 = ptau.setup(ctx, r1cs, make_ptau(ctx, 10, *toxic))
    blob, vkb = ptau.contribute(ctx, pk0, vk0, random.Random(4).randrange(2, R))
    pk = g16.ProvingKey(ctx, blob)
    rnd = random.Random(64)
    vals = [(rnd.randrange(R), rnd.randrange(R), rnd.randrange(1 << 160)) for _ in range(n)]
    recs = np.stack([circuit.pack_deposit_inputs(*v) for v in vals])
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(n)]
    proofs, pub = circuit.deposit_prove(ctx, pk, ctx.to_device(recs), rs, return_public=True)
    proofs, pub = np.asarray(proofs), np.asarray(pub)
    for t in range(n):
        assert g16.verify(vkb, pub[t], proofs[t].tobytes(), lib=ctx._lib) is True, t
    wrong = pub.copy()
    wrong[n // 2, 1, 0] ^= 1
    assert g16.verify(vkb, wrong[n // 2], proofs[n // 2].tobytes(), lib=ctx._lib) is False
    vk = g16.VerifyingKey(ctx, vkb)
    assert vk.verify_batch(pub, proofs).all()
    got = vk.verify_batch(wrong, proofs)
    assert not got[n // 2] and got.sum() == n - 1
    vk.close()
    wit = np.asarray(ctx.to_host(circuit.deposit_witness(ctx, ctx.to_device(recs[[0, n - 1]]))))
    ck = oc.prepared_key_from_blob(blob)
    assert proofs[0].tobytes() == ck.prove(wit[0], *rs[0]) and proofs[n - 1].tobytes() == ck.prove(wit[1], *rs[n - 1])
    pk.close()


# ---- 5: the file loop ----------------------------------------------------------------------------------------------------------
def case_file_round_trip(ctx, tmp_path=None):
    """.r1cs + .ptau -> key -> .zkey -> key: og_zkey_import (with the .r1cs) returns the ptau-made key's group elements; the CLI's
    `setup` writes exactly that file"""
    from owshen_amd import ptau, zkey as zk
    r1cs = _small(25, 3)
    toxic = _toxic(555)
    pdata = make_ptau(ctx, r1cs.log_d, *toxic)
    rdata = zk.write_r1cs(r1cs, lib=ctx._lib)
    pk, vk = ptau.setup(ctx, r1cs, pdata)
    zdata = zk.export_zkey(ctx, pk, vk)
    pk2, vk2 = zk.import_zkey(ctx, zdata, rdata)
    m, l, d = r1cs.n_wires, r1cs.n_pub, 1 << r1cs.log_d
    pad = lambda n: (n + 31) // 32 * 32                                                    # noqa: E731
    tail = pad(64 * m) * 2 + pad(128 * m) + pad(64 * (m - l - 1)) + pad(64 * (d - 1))
    assert vk2 == vk and pk2[-tail:] == pk[-tail:] and pk2[80:592] == pk[80:592]
    assert struct.unpack("<10Q", pk2[:80])[8] == 0                     # the C matrix rides along
    if tmp_path is not None:
        paths = [str(tmp_path / n) for n in ("c.r1cs", "pot.ptau", "out.zkey", "out_d.zkey")]
        for p, b in zip(paths, (rdata, pdata)):
            with open(p, "wb") as f:
                f.write(b)
        zk.main(["setup", paths[0], paths[1], paths[2]], ctx=ctx)
        assert open(paths[2], "rb").read() == zdata
        zk.main(["setup", paths[0], paths[1], paths[3], "--delta", "%x" % 0xabcdef123], ctx=ctx)
        assert open(paths[3], "rb").read() == zk.export_zkey(ctx, *ptau.contribute(ctx, pk, vk, 0xabcdef123))


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def f2_sqrt(a):
    """a square root in Fq2 = Fq[u] / (u^2 + 1), q = 3 mod 4, or None: (x0 + x1 u)^2 = a with x0^2 = (a0 +- sqrt(a0^2 + a1^2)) / 2"""
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (P + 1) // 4, P)
        if s * s % P == a0:
            return (s, 0)
        s = pow(-a0 % P, (P + 1) // 4, P)
        return (0, s) if s * s % P == -a0 % P else None
    n = pow((a0 * a0 + a1 * a1) % P, (P + 1) // 4, P)
    if n * n % P != (a0 * a0 + a1 * a1) % P:
        return None
    half = fields.inv(2, P)
    for s in (n, -n % P):
        t = (a0 + s) * half % P
        x0 = pow(t, (P + 1) // 4, P)
        if x0 and x0 * x0 % P == t:
            x1 = a1 * fields.inv(2 * x0 % P, P) % P
            assert fields.f2_sqr((x0, x1)) == (a0 % P, a1 % P)
            return (x0, x1)
    return None


def twist_point_outside_the_subgroup(seed=1):
    """a point of the twist y^2 = x^3 + 3 / (9 + u) for a random x: the cofactor is ~2^254, so it is outside the order-r subgroup"""
    rnd = random.Random(seed)
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = f2_sqrt(fields.f2_add(fields.f2_mul(fields.f2_sqr(x), x), G2_B))
        if y is not None:
            return x, y


def _replace(sections, sid, body):
    return [(s, body if s == sid else b) for s, b in sections]


def case_refusals(ctx):
    from owshen_amd import ptau
    from owshen_amd.api import OwshenGpuError
    r1cs = _small(25, 3)
    toxic = _toxic(66)
    sec = ptau_sections(ctx, 5, *toxic)
    body = dict(sec)
    ptau.setup(ctx, r1cs, _file(sec))

    def patched(sid, off, new):
        b = bytearray(body[sid])
        b[off:off + len(new)] = new
        return _file(_replace(sec, sid, bytes(b)))
    x, y = twist_point_outside_the_subgroup()
    rogue = _enc(b"".join(v.to_bytes(32, "little") for v in (x[0], x[1], y[0], y[1])))
    cases = {
        "wrong magic": (_file(sec, magic=b"ptax"), "not a ptau file"),
        "wrong q": (patched(1, 4, (P + 2).to_bytes(32, "little")), "section 1"),
        "power below the domain": (_file(ptau_sections(ctx, 4, *toxic)), "section 1"),
        "section 2 short": (_file(_replace(sec, 2, body[2][:-64])), "section 2"),
        "section 5 missing": (_file([s for s in sec if s[0] != 5]), "section 5"),
        "coordinate >= q": (patched(4, 64 * 3, P.to_bytes(32, "little")), "section 4"),
        "G1 point off the curve": (patched(5, 64 * 7 + 32, (12345).to_bytes(32, "little")), "section 5"),
        "tauG1[0] is not the generator": (patched(2, 0, body[2][64:128]), "section 2"),
        "tauG2[0] is not the generator": (patched(3, 0, body[3][128:256]), "section 3"),
        "tauG2 entry outside the subgroup": (patched(3, 128 * 9, rogue), "section 3"),
        "betaG2 outside the subgroup": (patched(6, 0, rogue), "section 6"),
        "empty": (b"", "not a ptau file"),
    }
    for name, (data, needle) in cases.items():
        with pytest.raises(OwshenGpuError) as e:
            ptau.setup(ctx, r1cs, data)
        assert e.value.code == -1, (name, e.value)
        assert "og_setup_ptau" in str(e.value) and needle in str(e.value), (name, str(e.value))
    assert "subgroup" in _reason(ctx, r1cs, cases["tauG2 entry outside the subgroup"][0])
    assert "generator" in _reason(ctx, r1cs, cases["tauG1[0] is not the generator"][0])
    assert "curve" in _reason(ctx, r1cs, cases["G1 point off the curve"][0])
    assert "modulus" in _reason(ctx, r1cs, cases["coordinate >= q"][0])
    # an entry past the used range is not looked at: the same rogue point at tauG2[d .. ] of a larger file
    big = ptau_sections(ctx, 6, *toxic)
    b3 = bytearray(dict(big)[3])
    b3[128 * 40:128 * 41] = rogue
    ptau.setup(ctx, r1cs, _file(_replace(big, 3, bytes(b3))))


def _reason(ctx, r1cs, data):
    from owshen_amd import ptau
    from owshen_amd.api import OwshenGpuError
    with pytest.raises(OwshenGpuError) as e:
        ptau.setup(ctx, r1cs, data)
    return str(e.value)


def case_null_handles(lib):
    """refused before any device is touched (runs on a host without one)"""
    import ctypes as C
    buf = (C.c_uint8 * 64)()
    p, n = C.c_void_p(), C.c_size_t()
    assert lib.og_setup_ptau(None, None, buf, 64, C.byref(p), C.byref(n), C.byref(p), C.byref(n)) == -1
    assert b"og_setup_ptau: null" in lib.og_last_error()
    assert lib.og_pk_contribute(None, buf, 64, buf, 64, buf, C.byref(p), C.byref(n), C.byref(p), C.byref(n)) == -1
    assert b"og_pk_contribute: null" in lib.og_last_error()
    info = (C.c_uint64 * 4)()
    assert lib.og_ptau_info(None, 0, info) == -1 and lib.og_ptau_info(buf, 64, None) == -1
    assert lib.og_ptau_info(buf, 64, info) == -1 and b"not a ptau file" in lib.og_last_error()


# ---- 8: host only -----------------------------------------------------------------------------------------------------------------
def case_info(ctx, lib):
    from owshen_amd import ptau
    sec = ptau_sections(ctx, 3, *_toxic(8))
    assert ptau.info(_file(sec), lib=lib) == {"power": 3, "ceremony_power": 3, "tau_g1_points": 15, "has_lagrange": False}
    more = sec + [(13, b"x"), (14, b""), (15, b"yy")]
    assert ptau.info(_file(more), lib=lib)["has_lagrange"] is True
    assert ptau.info(_file([s for s in sec if s[0] != 2]), lib=lib)["tau_g1_points"] == 0
