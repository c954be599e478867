"""og_claim_shape / og_claim_r1cs / og_claim_witness_d / og_claim_prove_batch_d and og_note_seal_owned_batch_d /
og_note_scan_owned_batch_d are declared in the header, have a ctypes signature, and are exported by the shipped library and by the hooks
library alike; the header states the scheme and the statement; the shape query needs no device.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"og_claim_shape": (r"int depth, uint64_t shape\[3\]", 2), "og_claim_r1cs": (r"og_ctx\* ctx, int depth, og_r1cs\*\* out", 3),
         "og_claim_witness_d": (r"og_ctx\* ctx, int depth, const uint8_t\* inputs_d, size_t n, uint8_t\* witness_out_d", 5),
         "og_claim_prove_batch_d": (r"og_ctx\* ctx, const og_pk\* pk, int depth, const uint8_t\* inputs_d, size_t n, const uint8_t\* rs,", 8),
         "og_note_seal_owned_batch_d": (r"og_ctx\* ctx, const uint8_t\* requests_d, size_t n, uint8_t\* memos_out_d, uint8_t\* notes_out_d, "
                                        r"uint32_t\* ok_out", 6),
         "og_note_scan_owned_batch_d": (r"og_ctx\* ctx, const uint8_t sk\[32\], const uint8_t\* memos_d, const uint8_t\* leaves_d, size_t n, "
                                        r"uint8_t\* opened_out_d, uint32_t\* hit_out", 7)}


def test_the_six_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib, api, circuit
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))
    for name, (args, n_args) in NAMES.items():
        assert re.search(r"^int %s\(%s" % (name, args), header, re.M), name
        assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
        assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
        assert hasattr(hooks, name), name
    assert hasattr(api.Context, "note_seal_owned") and hasattr(api.Context, "note_scan_owned")
    assert all(hasattr(circuit, f) for f in ("claim_shape", "claim_r1cs", "claim_r1cs_native", "claim_witness", "claim_prove", "pack_claim_inputs"))
    for word in ("tag = H(k, 6)", "t = H(k, 7)", "P = pk + t * BASE", "x = (sk + t) mod l", "nullifier_hash = H(x, 1)", "x < l", "2^251 - l",
                 "x3 (1 + d u_i v_i w3)", "field 0 if x >= l"):   # the scheme and the statement are stated in the header, not only named
        assert word in header, word


def test_shape_query_without_a_device():
    from owshen_amd import _lib, circuit
    from tests import claim_spec as spec
    shp = (C.c_uint64 * 3)()
    for depth, want in ((1, (6010, 6142)), (2, (6743, 6874)), (32, (28733, 28834)), (64, None)):
        assert _lib.lib.og_claim_shape(depth, shp) == 0
        assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == circuit.claim_shape(depth) and int(shp[2]) == 4
        assert want is None or spec.shape(depth) == want
    assert spec.shape(32)[1] + 4 + 1 <= 1 << 15, "the depth-32 statement leaves the 2^15 domain"
    for depth in (0, 65, -1):
        assert _lib.lib.og_claim_shape(depth, shp) == -1
    assert _lib.lib.og_claim_shape(32, None) == -1


def test_null_arguments_are_refused_before_the_device():
    from owshen_amd import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 160)()
    ok = (C.c_uint32 * 1)()
    null = C.c_void_p()
    assert lib.og_note_seal_owned_batch_d(null, buf, 1, buf, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_note_scan_owned_batch_d(null, buf, buf, buf, 1, buf, ok) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_claim_witness_d(null, 2, buf, 1, buf) == -1 and b"null og_ctx" in lib.og_last_error()
    assert lib.og_claim_prove_batch_d(null, null, 2, buf, 1, buf, buf, None) == -1
    assert lib.og_claim_r1cs(null, 2, None) == -1


def test_the_builders_compute_their_own_constants():
    """product code imports nothing from oracle/: the Python builder's curve constants are the oracle's, and its T_i the spec's"""
    from oracle.py import babyjubjub as bj
    from owshen_amd import circuit
    from tests import claim_spec as spec
    assert (circuit.ED_A, circuit.ED_D, circuit.ED_BASE, circuit.ED_L) == (bj.A, bj.D, bj.BASE, spec.ELL) and circuit.C_N_CMP == spec.N_CMP
    t = circuit.ED_BASE
    for want in spec.base_powers()[:12]:
        assert t == want
        t = circuit._ed_double(t)
    src = open(os.path.join(ROOT, "owshen_amd", "circuit.py")).read()
    assert "oracle" not in "".join(line for line in src.splitlines() if line.lstrip().startswith(("import ", "from ")))
