"""The OWPK0001 / OWVK0001 blobs at their consumers; cases shared by the CPU-interpreter run (test_emu_key_blob.py) and the GPU run
(test_gpu_key_blob.py).  The reader and the writer of the two formats live in owshen_amd/csrc/key_blob.h; what these cases pin is
that the entry points built on it take, refuse and produce exactly what they did when each of them parsed the blobs on its own:

  1. an outcome table -- malformed variants of a toy key crossed with the consumers: return code, the `og_...` prefix of the
     refusal, og_pk_verify's mask, and whether a proof still verifies after an accepted load -- against
     tests/golden/key_blob/outcomes.json, entry by entry;
  2. SHA-256 of every blob a writer makes, against tests/golden/key_blob/digests.json;
  3. the consumers with the caller's blobs at an odd address;
  4. og_pk_info against the blob's header.

Both JSON files are recordings (tests/golden/key_blob/README.md), made by `python -m tests.key_blob_cases`.

Two keys of og_setup with fixed toxic values.  K1: the 25-constraint circuit of tests/ptau_cases.py -- 29 QAP rows, so the row
pointers end off a 32-byte boundary, and so do the column sections of at least two matrices (asserted below): every padding of
the layout is exercised.  K2: one constraint over wire 0 alone -- domain 2, one H entry, and NO private wire: an empty L query.
Every malformed variant is one the library refuses on the host, compares with memcmp, or treats as plain field arithmetic;
none can make a kernel index out of bounds."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np

from oracle.py import fields
from tests import ptau_cases as pc
from tests.ptau_verify_cases import _canon, _put
from tests.r1cs_util import random_r1cs

R = fields.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_blob")
DELTA, CONTRIBUTION = 0x1234567890abcdef1234567, 0xabcdef123
_CACHE = {}

PK_CONSUMERS = ("og_pk_load", "og_zkey_export", "og_pk_contribute", "og_pk_verify")
VK_CONSUMERS = ("og_verify", "og_vk_load", "og_zkey_export", "og_pk_contribute", "og_pk_verify")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _wit(z):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(-1, 32).copy()


class Material:
    """K1 with its file, its circuit handle and one proof; K2"""

    def __init__(self, ctx):
        from owshen_amd import groth16 as g16
        self.r1cs = pc._small(25, 3)
        toxic = pc._toxic(125)
        self.ptau = pc.make_ptau(ctx, self.r1cs.log_d, *toxic)
        pk, vk = g16.setup(ctx, self.r1cs, *toxic, 1, DELTA)                # gamma = 1: a key of the file, for og_pk_verify
        self.pk, self.vk = pk, g16.vk_to_bytes(vk)
        _n, _cons, z0 = random_r1cs(25, 3, seed=25 + 5000)
        self.wit = _wit(z0)
        self.pub = self.wit[1:4].copy()
        key = g16.ProvingKey(ctx, self.pk)
        self.proof = bytes(key.prove(self.wit, 11, 12))
        key.close()
        assert g16.verify(self.vk, self.pub, self.proof, lib=ctx._lib) is True
        rc, self.r1cs_h, self._keep = g16._r1cs_handle(ctx._lib, self.r1cs)
        assert rc == 0
        one = {0: 1}
        self.r1cs2 = g16.R1CS.from_constraints(1, 0, [(one, one, one)])
        pk2, vk2 = g16.setup(ctx, self.r1cs2, 101, 202, 303, 404, 505)
        self.pk2, self.vk2 = pk2, g16.vk_to_bytes(vk2)


def material(ctx):
    if id(ctx) not in _CACHE:
        _CACHE[id(ctx)] = (ctx, Material(ctx))
    return _CACHE[id(ctx)][1]


def _header(pk):
    return struct.unpack("<10Q", pk[:80])


def _word(pk, k, value):
    return _put(pk, 8 * k, struct.pack("<Q", value))


def _csr(pk):
    """offsets of ptr | col | val of A, B, C"""
    _magic, _m, _l, _power, n_rows, *nnz = _header(pk)[:8]
    pad = lambda n: (n + 31) // 32 * 32                                                    # noqa: E731
    off, out = 592, []
    for k in range(3):
        out.append((off, off + pad(4 * (n_rows + 1)), off + pad(4 * (n_rows + 1)) + pad(4 * nnz[k])))
        off = out[-1][2] + pad(32 * nnz[k])
    return out


def case_k1_meets_every_padding(ctx):
    mat = material(ctx)
    _magic, m, l, power, n_rows, *nnz = _header(mat.pk)[:8]
    assert (m, l, power, n_rows) == (32, 3, 5, 29) and (n_rows + 1) % 8 != 0
    assert sum(1 for n in nnz if n % 8 != 0) >= 2 and all(nnz)
    assert _header(mat.pk2)[1:5] == (1, 0, 1, 2)                       # m - l - 1 = 0: no L entry; d - 1 = 1: one H entry


# ---- the variants ---------------------------------------------------------------------------------------------------------------
def pk_variants(ctx):
    mat = material(ctx)
    pk = mat.pk
    _magic, m, _l, power, n_rows, nnz_a, _nnz_b, nnz_c = _header(pk)[:8]
    (ptr_a, col_a, val_a), _b, (_ptr_c, col_c, _val_c) = _csr(pk)
    ptr = list(struct.unpack("<%dI" % (n_rows + 1), pk[ptr_a:ptr_a + 4 * (n_rows + 1)]))
    i = next(i for i in range(1, n_rows - 1) if ptr[i] < ptr[i + 1])
    swapped = ptr[:i] + [ptr[i + 1], ptr[i]] + ptr[i + 2:]
    assert nnz_c > 0 and swapped[i] > swapped[i + 1] and max(swapped) <= nnz_a
    u32 = lambda v: struct.pack("<I", v)                                                   # noqa: E731
    return {
        "valid": pk,
        "wrong magic": _put(pk, 0, b"OWPK0002"),
        "length 591": pk[:591],
        "m = 0": _word(pk, 1, 0),
        "l = m": _word(pk, 2, m),
        "m = 2^31": _word(pk, 1, 1 << 31),
        "log_d = 0": _word(pk, 3, 0),
        "log_d = 28": _word(pk, 3, 28),
        "log_d = 29": _word(pk, 3, 29),
        "n_rows = d + 1": _word(pk, 4, (1 << power) + 1),
        "nnz_a = 2^32": _word(pk, 5, 1 << 32),
        "nnz_a + 1": _word(pk, 5, nnz_a + 1),
        "word 8 = 1 beside a C matrix": _word(pk, 8, 1),
        "word 8 = 2": _word(pk, 8, 2),
        "word 9 = 1": _word(pk, 9, 1),
        "cut by 32 bytes": pk[:-32],
        "extended by 32 bytes": pk + bytes(32),
        "ptr_a[0] = 1": _put(pk, ptr_a, u32(1)),
        "a descending pair in ptr_a": _put(pk, ptr_a, struct.pack("<%dI" % (n_rows + 1), *swapped)),
        "ptr_a[n_rows] != nnz_a": _put(pk, ptr_a + 4 * n_rows, u32(nnz_a - 1)),
        "a column of A equal to m": _put(pk, col_a, u32(m)),
        "a column of C equal to m": _put(pk, col_c, u32(m)),
        "a value of A equal to r": _put(pk, val_a, R.to_bytes(32, "little")),
    }


def vk_variants(ctx):
    mat = material(ctx)
    vk = mat.vk
    n_pub = struct.unpack("<Q", vk[8:16])[0]
    return {
        "valid": vk,
        "wrong magic": _put(vk, 0, b"OWVK0002"),
        "n_pub + 1": _put(vk, 8, struct.pack("<Q", n_pub + 1)),
        "64 bytes short": vk[:-64],
        "64 bytes long": vk + bytes(64),
        "n_pub = 2^24 + 1": _put(vk, 8, struct.pack("<Q", (1 << 24) + 1)),
        "another alpha": _put(vk, 16, _canon(ctx, 1, [987654321])),
        "another delta2": _put(vk, 16 + 64 + 256, _canon(ctx, 2, [123456789])),
    }


# ---- the consumers, through the C ABI, with the blobs `shift` bytes into their buffers ------------------------------------------
def _at(data, shift):
    buf = (C.c_uint8 * (len(data) + shift + 1))()
    C.memmove(C.addressof(buf) + shift, data, len(data))
    return buf, C.c_void_p(C.addressof(buf) + shift)


def _outcome(lib, rc, **more):
    out = {"rc": rc, "prefix": lib.og_last_error().decode("utf-8", "replace").split(":")[0] if rc else None}
    out.update(more)
    return out


def _take(lib, p, n):
    from owshen_amd.zkey import _take as take
    return take(lib, p, n)


def call_pk_load(ctx, pk, vk, shift=0, prove=True):
    """-> (outcome, the loaded key's og_pk_info); `proof`: what becomes of K1's witness under the loaded key"""
    from owshen_amd import groth16 as g16
    from owshen_amd.api import OwshenGpuError
    mat, lib = material(ctx), ctx._lib
    _keep, p = _at(pk, shift)
    h = C.c_void_p()
    rc = lib.og_pk_load(ctx._h, p, len(pk), C.byref(h))
    if rc:
        return _outcome(lib, rc, proof=None), None
    key = g16.ProvingKey.__new__(g16.ProvingKey)
    key.ctx, key._h = ctx, h
    info = (C.c_uint64 * 4)()
    assert lib.og_pk_info(h, info) == 0
    key.n_wires, key.n_pub, key.log_d, key.n_rows = (int(x) for x in info)
    proof = None
    try:
        if prove:
            proof = "verifies" if g16.verify(mat.vk, mat.pub, bytes(key.prove(mat.wit, 11, 12)), lib=lib) else "does not verify"
    except OwshenGpuError:
        proof = "refused"
    key.close()
    return _outcome(lib, 0, proof=proof), tuple(int(x) for x in info)


def call_zkey_export(ctx, pk, vk, shift=0):
    lib = ctx._lib
    _k1, p = _at(pk, shift)
    _k2, v = _at(vk, shift)
    z_p, z_n = C.c_void_p(), C.c_size_t()
    ctx._pre()
    rc = lib.og_zkey_export(ctx._h, p, len(pk), v, len(vk), C.byref(z_p), C.byref(z_n))
    return _outcome(lib, rc), None if rc else _take(lib, z_p, z_n)


def call_pk_contribute(ctx, pk, vk, shift=0):
    lib = ctx._lib
    _k1, p = _at(pk, shift)
    _k2, v = _at(vk, shift)
    _k3, d = _at(CONTRIBUTION.to_bytes(32, "little"), shift)
    pk_p, vk_p, pk_n, vk_n = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    ctx._pre()
    rc = lib.og_pk_contribute(ctx._h, p, len(pk), v, len(vk), d, C.byref(pk_p), C.byref(pk_n), C.byref(vk_p), C.byref(vk_n))
    return _outcome(lib, rc), None if rc else (_take(lib, pk_p, pk_n), _take(lib, vk_p, vk_n))


def call_pk_verify(ctx, pk, vk, shift=0):
    mat, lib = material(ctx), ctx._lib
    _k1, p = _at(pk, shift)
    _k2, v = _at(vk, shift)
    _k3, f = _at(mat.ptau, shift)
    failed = C.c_uint32(0xffffffff)
    ctx._pre()
    rc = lib.og_pk_verify(ctx._h, mat.r1cs_h, f, len(mat.ptau), p, len(pk), v, len(vk), C.byref(failed))
    return _outcome(lib, rc, mask=None if rc else int(failed.value)), None


def call_verify(ctx, pk, vk, shift=0):
    mat, lib = material(ctx), ctx._lib
    _k1, v = _at(vk, shift)
    _k2, pub = _at(mat.pub.tobytes(), shift)
    _k3, proof = _at(mat.proof, shift)
    ok = C.c_int(-1)
    rc = lib.og_verify(v, len(vk), pub, mat.pub.shape[0], proof, C.byref(ok))
    return _outcome(lib, rc, proof=None if rc else bool(ok.value)), None


def call_vk_load(ctx, pk, vk, shift=0):
    from owshen_amd import groth16 as g16
    mat, lib = material(ctx), ctx._lib
    _k1, v = _at(vk, shift)
    h = C.c_void_p()
    ctx._pre()
    rc = lib.og_vk_load(ctx._h, v, len(vk), C.byref(h))
    if rc:
        return _outcome(lib, rc, proof=None), None
    key = g16.VerifyingKey.__new__(g16.VerifyingKey)
    key.ctx, key._h = ctx, h
    info = (C.c_uint64 * 4)()
    assert lib.og_vk_info(h, info) == 0
    key.n_pub = int(info[0])
    ok = bool(key.verify_batch(mat.pub[None], np.frombuffer(mat.proof, np.uint8)[None])[0])
    key.close()
    return _outcome(lib, 0, proof=ok), None


CALLS = {"og_pk_load": call_pk_load, "og_zkey_export": call_zkey_export, "og_pk_contribute": call_pk_contribute, "og_pk_verify": call_pk_verify,
         "og_verify": call_verify, "og_vk_load": call_vk_load}


# ---- 1: the outcome table -------------------------------------------------------------------------------------------------------
def outcomes(ctx, blob, consumer):
    """{"<blob> | <consumer> | <variant>": outcome} for one consumer of the proving-key ("pk") or verifying-key ("vk") variants"""
    mat = material(ctx)
    out = {}
    for name, bad in (pk_variants(ctx) if blob == "pk" else vk_variants(ctx)).items():
        pair = (bad, mat.vk) if blob == "pk" else (mat.pk, bad)
        out["%s | %s | %s" % (blob, consumer, name)] = CALLS[consumer](ctx, *pair)[0]
    return out


def case_outcomes(ctx, blob, consumer):
    got = outcomes(ctx, blob, consumer)
    want = {k: v for k, v in golden("outcomes.json").items() if k.startswith("%s | %s | " % (blob, consumer))}
    assert len(want) == (23 if blob == "pk" else 8) and sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


# ---- 2: bytes -------------------------------------------------------------------------------------------------------------------
def digests(ctx):
    from owshen_amd import ptau, zkey as zk
    mat = material(ctx)
    made = {"og_setup K1": (mat.pk, mat.vk), "og_setup K2": (mat.pk2, mat.vk2), "og_setup_ptau K1": ptau.setup(ctx, mat.r1cs, mat.ptau),
            "og_pk_contribute K1": call_pk_contribute(ctx, mat.pk, mat.vk)[1]}
    zkey = call_zkey_export(ctx, mat.pk, mat.vk)[1]
    made["og_zkey_import flag 1"] = zk.import_zkey(ctx, zkey)
    made["og_zkey_import flag 0"] = zk.import_zkey(ctx, zkey, zk.write_r1cs(mat.r1cs, lib=ctx._lib))
    assert _header(made["og_zkey_import flag 1"][0])[8] == 1 and _header(made["og_zkey_import flag 0"][0])[8] == 0
    out = {"og_zkey_export K1 zkey": hashlib.sha256(zkey).hexdigest()}
    for name, (pk, vk) in made.items():
        out[name + " pk"], out[name + " vk"] = hashlib.sha256(pk).hexdigest(), hashlib.sha256(vk).hexdigest()
    return out


def case_digests(ctx):
    got, want = digests(ctx), golden("digests.json")
    assert len(want) == 13 and got == want


# ---- 3: a caller's buffer has no alignment ----------------------------------------------------------------------------------------
def case_unaligned(ctx, consumer):
    """the blobs one byte into their buffers: the same outcome, the same bytes out"""
    mat = material(ctx)
    aligned, odd = CALLS[consumer](ctx, mat.pk, mat.vk, 0), CALLS[consumer](ctx, mat.pk, mat.vk, 1)
    assert aligned[0]["rc"] == 0 and odd == aligned
    if consumer in ("og_pk_load", "og_verify", "og_vk_load"):
        assert aligned[0]["proof"] in ("verifies", True)
    if consumer == "og_pk_verify":
        assert aligned[0]["mask"] == 0


# ---- 4: og_pk_info ----------------------------------------------------------------------------------------------------------------
def case_pk_info(ctx):
    mat = material(ctx)
    for pk in (mat.pk, mat.pk2):
        out, info = call_pk_load(ctx, pk, mat.vk, prove=False)
        assert out["rc"] == 0 and info == _header(pk)[1:5]


def record(ctx):
    """writes the two recordings from what THIS build does (tests/golden/key_blob/README.md)"""
    table = {}
    for blob, consumers in (("pk", PK_CONSUMERS), ("vk", VK_CONSUMERS)):
        for consumer in consumers:
            table.update(outcomes(ctx, blob, consumer))
    os.makedirs(GOLDEN, exist_ok=True)
    for name, data in (("outcomes.json", table), ("digests.json", digests(ctx))):
        with open(os.path.join(GOLDEN, name), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(os.path.join(GOLDEN, "k1_pk.bin"), "wb") as f:
        f.write(material(ctx).pk)


if __name__ == "__main__":
    from tests import emu
    record(emu.Ctx())
