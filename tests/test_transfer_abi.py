"""og_transfer_shape / og_transfer_r1cs / og_transfer_witness_d / og_transfer_prove_batch_d are declared in the header, have a ctypes
signature, and are exported by the shipped library and by the hooks library alike; the shape query needs no device.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"og_transfer_shape": (r"int depth, uint64_t shape\[3\]", 2), "og_transfer_r1cs": (r"og_ctx\* ctx, int depth, og_r1cs\*\* out", 3),
         "og_transfer_witness_d": (r"og_ctx\* ctx, int depth, const uint8_t\* inputs_d, size_t n, uint8_t\* witness_out_d", 5),
         "og_transfer_prove_batch_d": (r"og_ctx\* ctx, const og_pk\* pk, int depth, const uint8_t\* inputs_d, size_t n, const uint8_t\* rs,", 8)}


def test_the_four_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))
    for name, (args, n_args) in NAMES.items():
        assert re.search(r"^int %s\(%s" % (name, args), header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
        assert hasattr(hooks, name), name


def test_shape_query_without_a_device():
    from owshen_amd import _lib, circuit
    from tests import transfer_spec as spec
    shp = (C.c_uint64 * 3)()
    for depth, want in ((1, (6840, 6832)), (2, (7573, 7564)), (32, (29563, 29524)), (64, None)):
        assert _lib.lib.og_transfer_shape(depth, shp) == 0
        assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.transfer_shape(depth) and int(shp[2]) == 5
        assert want is None or spec.shape(depth) == want
    for depth in (0, 65, -1):
        assert _lib.lib.og_transfer_shape(depth, shp) == -1
    assert _lib.lib.og_transfer_shape(32, None) == -1
