"""og_note_seal_batch_d / og_note_scan_batch_d are declared in the header, have a ctypes signature, and are exported by the shipped
library and by the hooks library alike; null arguments are refused before any device call, n = 0 needs no pointer, a non-canonical sk is
OG_ERR_INVALID; the seam og_hook_ed_mul_uniform_d is in the hooks library only.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NAMES = {"og_note_seal_batch_d": (r"og_ctx\* ctx, const uint8_t\* requests_d, size_t n, uint8_t\* memos_out_d, uint8_t\* notes_out_d, uint32_t\* ok_out", 6),
         "og_note_scan_batch_d": (r"og_ctx\* ctx, const uint8_t sk\[32\], const uint8_t\* memos_d, const uint8_t\* leaves_d, size_t n, "
                                  r"uint8_t\* opened_out_d, uint32_t\* hit_out", 7)}
SEAM = "og_hook_ed_mul_uniform_d"


def _hooks():
    from owshen_amd import _lib
    return C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))


def test_the_two_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib, api
    from oracle.py.fields import R as oracle_r
    assert R == oracle_r == api.FR_MODULUS
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = _hooks()
    for name, (args, n_args) in NAMES.items():
        assert re.search(r"^int %s\(%s\);" % (name, args), header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
        assert hasattr(hooks, name), name
    assert hasattr(api.Context, "note_seal") and hasattr(api.Context, "note_scan")
    for word in ("tag = H(k, 1)", "small(E)", "hit = 2"):   # the scheme is stated in the header, not only named
        assert word in header, word


def test_null_arguments_are_refused_before_the_device():
    """no device exists where this runs: OG_ERR_INVALID (-1), never OG_ERR_HIP or OG_ERR_NO_DEVICE"""
    from owshen_amd import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 160)()
    ok = (C.c_uint32 * 1)()
    null = C.c_void_p()
    assert lib.og_note_seal_batch_d(null, buf, 1, buf, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_note_scan_batch_d(null, buf, buf, buf, 1, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_note_seal_batch_d(null, None, 0, None, None, None) == -1   # n = 0 still needs a handle


def _emu():
    from tests import emu
    return emu.lib


def test_pointer_and_sk_checks_on_a_live_context():
    """on the interpreter's build of the same capi.hip (a context exists there without a GPU): each required pointer on its own, n = 0
    with no pointer at all, leaves and opened rows optional, sk >= r named in the error"""
    lib = _emu()
    h = C.c_void_p()
    assert lib.og_init(0, C.byref(h)) == 0
    try:
        buf = (C.c_uint8 * 160)()
        out = (C.c_uint8 * 160)()
        ok = (C.c_uint32 * 1)()
        sk = (C.c_uint8 * 32)(1)
        seal, scan = lib.og_note_seal_batch_d, lib.og_note_scan_batch_d
        for args in ((None, 1, out, out, ok), (buf, 1, None, out, ok), (buf, 1, out, None, ok), (buf, 1, out, out, None)):
            assert seal(h, *args) == -1 and b"og_note_seal_batch_d: null argument" in lib.og_last_error(), args
        for args in ((None, buf, buf, 1, out, ok), (sk, None, buf, 1, out, ok), (sk, buf, buf, 1, out, None)):
            assert scan(h, *args) == -1 and b"og_note_scan_batch_d: null argument" in lib.og_last_error(), args
        assert seal(h, None, 0, None, None, None) == 0 and scan(h, None, None, None, 0, None, None) == 0
        for bad in (R, R + 1, (1 << 256) - 1):
            skb = (C.c_uint8 * 32).from_buffer_copy(bad.to_bytes(32, "little"))
            assert scan(h, skb, buf, None, 1, None, ok) == -1 and b"sk" in lib.og_last_error() and b"canonical" in lib.og_last_error()
        top = (C.c_uint8 * 32).from_buffer_copy((R - 1).to_bytes(32, "little"))
        for leaves, opened in ((None, None), (buf, None), (None, out), (buf, out)):   # an all-zero memo: E = (0, 0) is off the curve
            ok[0] = 7
            assert scan(h, top, buf, leaves, 1, opened, ok) == 0 and ok[0] == 0
    finally:
        lib.og_shutdown(h)


def test_the_seam_is_in_the_hooks_library_only():
    from owshen_amd import _lib
    hooks = _hooks()
    assert hasattr(hooks, SEAM), f"{SEAM} missing from the hooks build"
    assert not hasattr(_lib.lib, SEAM), f"{SEAM} is in the shipped library"
    assert "og_hook_" not in open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    fn = getattr(hooks, SEAM)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    buf = (C.c_uint8 * 64)()
    ok = (C.c_uint32 * 1)()
    assert fn(None, buf, buf, 1, buf, ok) == -1
