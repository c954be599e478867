"""og_note_seal_view_batch_d / og_note_scan_view_batch_d / og_note_unlock_batch_d are declared in the header, have a ctypes signature
and an api.Context method, and are exported by the shipped library and by the hooks library alike; the header states the scheme; a
null handle is refused before the device.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"og_note_seal_view_batch_d": (r"og_ctx\* ctx, const uint8_t\* requests_d, size_t n, uint8_t\* memos_out_d, uint8_t\* notes_out_d, "
                                       r"uint32_t\* ok_out\);", 6),
         "og_note_scan_view_batch_d": (r"og_ctx\* ctx, const uint8_t v\[32\], const uint8_t ps\[64\], const uint8_t\* memos_d, "
                                       r"const uint8_t\* leaves_d, size_t n, uint8_t\* opened_out_d, uint32_t\* hit_out\);", 8),
         "og_note_unlock_batch_d": (r"og_ctx\* ctx, const uint8_t sk\[32\], const uint8_t\* rows_d, const uint8_t\* leaves_d, size_t n, "
                                    r"uint8_t\* unlocked_out_d, uint32_t\* ok_out\);", 7)}


def test_the_three_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib, api
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))
    for name, (args, n_args) in NAMES.items():
        assert re.search(r"^int %s\(%s" % (name, args), header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
        assert hasattr(hooks, name), name
    assert all(callable(getattr(api.Context, m, None)) for m in ("note_seal_view", "note_scan_view", "note_unlock"))
    for word in ("tag = H(k, 10)", "t = H(k, 11)", "pad_a = H(k, 12)", "pad_t = H(k, 13)", "e | PV.x | PV.y | PS.x | PS.y | amount | token",
                 "S = e * PV", "P = PS + t * BASE", "t | amount | token | c", "x = (sk + t) mod l", "x | amount | token | c",
                 "small(PS)", "tests/view_note_spec.py"):   # the scheme is stated in the header, not only named
        assert word in header, word


def test_the_interpreter_context_has_the_methods():
    """tests/emu.Ctx takes them from api.Context: nothing to add there"""
    from owshen_amd import api
    src = open(os.path.join(ROOT, "tests", "emu.py")).read()
    assert "class Ctx(api.Context)" in src and "note_" not in src
    assert {"note_seal_view", "note_scan_view", "note_unlock"} <= set(vars(api.Context))


def test_a_null_handle_is_refused_before_the_device():
    from owshen_amd import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 224)()
    ok = (C.c_uint32 * 1)()
    null = C.c_void_p()
    assert lib.og_note_seal_view_batch_d(null, buf, 1, buf, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_note_scan_view_batch_d(null, buf, buf, buf, buf, 1, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_note_unlock_batch_d(null, buf, buf, buf, 1, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    # n = 0 with no handle is still a null handle: the handle is looked at first
    assert lib.og_note_unlock_batch_d(null, None, None, None, 0, None, None) == -1 and b"null og_ctx" in lib.og_last_error()
