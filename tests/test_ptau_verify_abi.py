"""og_ptau_verify / og_pk_verify are declared in the header, have a ctypes signature, and are exported by the shipped library and
by the hooks library alike; a null handle is refused before any device is touched.  No GPU."""
import ctypes as C
import os
import re

from tests import ptau_verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("og_ptau_verify", "og_pk_verify")


def test_the_two_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(og_ctx\* ctx, " % name, header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1]
    assert len(_abi.SIGNATURES["og_ptau_verify"][1]) == 4 and len(_abi.SIGNATURES["og_pk_verify"][1]) == 9
    hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))
    for name in NAMES:
        assert hasattr(hooks, name), name


def test_python_names_the_checks_in_mask_order():
    from owshen_amd import ptau
    assert ptau._names(0, ptau.PTAU_CHECKS) == [] and ptau._names(1 | 16, ptau.PTAU_CHECKS) == ["tauG1", "betaG2"]
    assert ptau._names(63, ptau.KEY_CHECKS) == ["header", "queries", "ic", "delta", "L", "H"]
    assert len(ptau.PTAU_CHECKS) == 5


def test_null_arguments_are_refused_without_a_device():
    from owshen_amd import _lib
    cases.case_null_handles(_lib.lib)
