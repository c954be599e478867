"""og_eddsa_pubkey_batch_d / og_eddsa_decompress_batch_d / og_eddsa_sign_batch_d / og_eddsa_verify_compressed_batch_d are declared in
the header, have a ctypes signature, and are exported by the shipped library and by the hooks library alike; null arguments are
refused before any device call; the two seams (og_hook_fr_sqrt_d, og_hook_ed_sign_s_d) are in the hooks library only.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"og_eddsa_pubkey_batch_d": (r"og_ctx\* ctx, const uint8_t\* sk_d, size_t n, uint8_t\* pk_out_d, uint8_t\* pkc_out_d, uint32_t\* ok_out", 6),
         "og_eddsa_decompress_batch_d": (r"og_ctx\* ctx, const uint8_t\* pkc_d, size_t n, uint8_t\* pk_out_d, uint32_t\* ok_out", 5),
         "og_eddsa_sign_batch_d": (r"og_ctx\* ctx, const uint8_t\* requests_d, size_t n, uint8_t\* records_out_d, uint32_t\* ok_out", 5),
         "og_eddsa_verify_compressed_batch_d": (r"og_ctx\* ctx, const uint8_t\* records_d, size_t n, uint32_t\* ok_out", 4)}
SEAMS = ("og_hook_fr_sqrt_d", "og_hook_ed_sign_s_d")


def _hooks():
    from owshen_amd import _lib
    return C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))


def test_the_four_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = _hooks()
    for name, (args, n_args) in NAMES.items():
        assert re.search(r"^int %s\(%s\);" % (name, args), header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
        assert hasattr(hooks, name), name
    assert "stays on the host" not in header   # the sentence the header had while decompression was the caller's


def test_null_arguments_are_refused_before_the_device():
    """no device exists where this runs: OG_ERR_INVALID (-1), never OG_ERR_HIP or OG_ERR_NO_DEVICE, and n = 0 needs no pointer"""
    from owshen_amd import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 192)()
    ok = (C.c_uint32 * 1)()
    null = C.c_void_p()
    for call in (lambda c, p, o: lib.og_eddsa_pubkey_batch_d(c, p, 1, buf, buf, o),
                 lambda c, p, o: lib.og_eddsa_decompress_batch_d(c, p, 1, buf, o),
                 lambda c, p, o: lib.og_eddsa_sign_batch_d(c, p, 1, buf, o),
                 lambda c, p, o: lib.og_eddsa_verify_compressed_batch_d(c, p, 1, o)):
        assert call(null, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    # a context that is no context is never dereferenced either: the pointer checks come before the lock and the device
    h = C.c_void_p()
    if lib.og_device_count() > 0:
        assert lib.og_init(0, C.byref(h)) == 0
        try:
            assert lib.og_eddsa_pubkey_batch_d(h, None, 1, buf, buf, ok) == -1 and b"null argument" in lib.og_last_error()
            assert lib.og_eddsa_pubkey_batch_d(h, buf, 1, buf, buf, None) == -1
            assert lib.og_eddsa_decompress_batch_d(h, None, 1, buf, ok) == -1 and lib.og_eddsa_decompress_batch_d(h, buf, 1, None, ok) == -1
            assert lib.og_eddsa_decompress_batch_d(h, buf, 1, buf, None) == -1
            assert lib.og_eddsa_sign_batch_d(h, None, 1, buf, ok) == -1 and lib.og_eddsa_sign_batch_d(h, buf, 1, None, ok) == -1
            assert lib.og_eddsa_sign_batch_d(h, buf, 1, buf, None) == -1
            assert lib.og_eddsa_verify_compressed_batch_d(h, None, 1, ok) == -1 and lib.og_eddsa_verify_compressed_batch_d(h, buf, 1, None) == -1
            for rc in (lib.og_eddsa_pubkey_batch_d(h, None, 0, None, None, None), lib.og_eddsa_decompress_batch_d(h, None, 0, None, None),
                       lib.og_eddsa_sign_batch_d(h, None, 0, None, None), lib.og_eddsa_verify_compressed_batch_d(h, None, 0, None)):
                assert rc == 0
        finally:
            lib.og_shutdown(h)


def test_the_seams_are_in_the_hooks_library_only():
    from owshen_amd import _lib
    hooks = _hooks()
    for seam in SEAMS:
        assert hasattr(hooks, seam), f"{seam} missing from the hooks build"
        assert not hasattr(_lib.lib, seam), f"{seam} is in the shipped library"
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    assert "og_hook_" not in header
    # and they refuse null arguments like everything else
    ok = (C.c_uint32 * 1)()
    buf = (C.c_uint8 * 96)()
    for seam in SEAMS:
        fn = getattr(hooks, seam)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        assert fn(None, buf, 1, buf, ok) == -1
