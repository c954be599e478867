"""Host-side mirror of the ceremony entry points of include/owshen_gpu.h (og_ptau_info / og_setup_ptau / og_pk_contribute /
og_ptau_verify / og_pk_verify, owshen_amd/csrc/ptau.hip): an R1CS and a powers-of-tau file become this library's proving /
verifying key blobs without a secret scalar in the process, one scalar turns such a key into a contributed one, and a file or
a key somebody else made can be checked before it is trusted.  No reference counterpart.  Every conversion and
every group operation happens inside the library.

    pk_blob, vk_blob = ptau.setup(ctx, zkey.read_r1cs(open("circuit.r1cs", "rb").read()), open("pot.ptau", "rb").read())
    pk_blob, vk_blob = ptau.contribute(ctx, pk_blob, vk_blob, secrets.randbelow(FR_MODULUS - 1) + 1)    # and forget it
    open("circuit_final.zkey", "wb").write(zkey.export_zkey(ctx, pk_blob, vk_blob))
    assert ptau.verify(ctx, pot) == [] and ptau.verify_key(ctx, r1cs, pot, pk_blob, vk_blob) == []   # a foreign file, a foreign key
"""
import ctypes as C

from .zkey import _lib_or_default, _raise, _take


# bit k of og_ptau_verify's / og_pk_verify's mask (include/owshen_gpu.h)
PTAU_CHECKS = ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")
KEY_CHECKS = ("header", "queries", "ic", "delta", "L", "H")


def _buf(data):
    data = bytes(data)
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0"), len(data)


def info(data, lib=None):
    """.ptau bytes -> dict(power, ceremony_power, tau_g1_points, has_lagrange); host only, no context"""
    lib = _lib_or_default(lib)
    buf, n = _buf(data)
    out = (C.c_uint64 * 4)()
    rc = lib.og_ptau_info(buf, n, out)
    if rc:
        _raise(lib, rc)
    return {"power": int(out[0]), "ceremony_power": int(out[1]), "tau_g1_points": int(out[2]), "has_lagrange": bool(out[3])}


def setup(ctx, r1cs, data):
    """owshen_amd.groth16.R1CS + .ptau bytes -> (OWPK0001 bytes, OWVK0001 bytes) with gamma = delta = 1 (snarkjs' initial zkey)"""
    from . import groth16
    lib = ctx._lib
    rc, h, _keep = groth16._r1cs_handle(lib, r1cs)
    ctx._check(rc)
    try:
        buf, n = _buf(data)
        pk_p, vk_p, pk_n, vk_n = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        ctx._pre()
        ctx._check(lib.og_setup_ptau(ctx._h, h, buf, n, C.byref(pk_p), C.byref(pk_n), C.byref(vk_p), C.byref(vk_n)))
    finally:
        lib.og_r1cs_free(h)
    pk = _take(lib, pk_p, pk_n)
    return pk, _take(lib, vk_p, vk_n)


def contribute(ctx, pk_blob, vk_blob, delta):
    """the delta step: (OWPK0001, OWVK0001) and a scalar 0 < delta < r (an int, or its 32 little-endian bytes) -> the pair with
    delta multiplied in.  The scalar is the caller's secret to draw and to forget; the library draws none."""
    lib = ctx._lib
    d = bytes(delta) if isinstance(delta, (bytes, bytearray)) else int(delta).to_bytes(32, "little")
    if len(d) != 32:
        raise ValueError("delta is 32 little-endian bytes")
    pk, pk_len = _buf(pk_blob)
    vk, vk_len = _buf(vk_blob)
    db, _ = _buf(d)
    pk_p, vk_p, pk_n, vk_n = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    ctx._pre()
    ctx._check(lib.og_pk_contribute(ctx._h, pk, pk_len, vk, vk_len, db, C.byref(pk_p), C.byref(pk_n), C.byref(vk_p), C.byref(vk_n)))
    out = _take(lib, pk_p, pk_n)
    return out, _take(lib, vk_p, vk_n)


def _names(mask, names):
    return [n for k, n in enumerate(names) if mask >> k & 1]


def verify_mask(ctx, data):
    """og_ptau_verify's mask for .ptau bytes: 0 = every section is a geometric sequence in the ratio tauG2[1] carries"""
    lib = ctx._lib
    buf, n = _buf(data)
    failed = C.c_uint32(0xffffffff)
    ctx._pre()
    ctx._check(lib.og_ptau_verify(ctx._h, buf, n, C.byref(failed)))
    return int(failed.value)


def verify(ctx, data):
    """.ptau bytes -> the names of the failed checks (PTAU_CHECKS), [] if the file is a valid ceremony.  A malformed file raises."""
    return _names(verify_mask(ctx, data), PTAU_CHECKS)


def verify_key_mask(ctx, r1cs, data, pk_blob, vk_blob):
    """og_pk_verify's mask: 0 = (pk, vk) is the key of `r1cs` (owshen_amd.groth16.R1CS) from the .ptau `data`, up to its delta"""
    from . import groth16
    lib = ctx._lib
    rc, h, _keep = groth16._r1cs_handle(lib, r1cs)
    ctx._check(rc)
    try:
        buf, n = _buf(data)
        pk, pk_len = _buf(pk_blob)
        vk, vk_len = _buf(vk_blob)
        failed = C.c_uint32(0xffffffff)
        ctx._pre()
        ctx._check(lib.og_pk_verify(ctx._h, h, buf, n, pk, pk_len, vk, vk_len, C.byref(failed)))
    finally:
        lib.og_r1cs_free(h)
    return int(failed.value)


def verify_key(ctx, r1cs, data, pk_blob, vk_blob):
    """-> the names of the failed checks (KEY_CHECKS), [] if the key is this circuit's key from this ceremony"""
    return _names(verify_key_mask(ctx, r1cs, data, pk_blob, vk_blob), KEY_CHECKS)
