"""og_send_* and og_redeem_* (shape, r1cs, witness_d, prove_batch_d each) are declared in the header, have a ctypes signature, and are
exported by the shipped library and by the hooks library alike; the header states both statements; the shape queries need no device.
No GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATEMENTS = ("send", "redeem")
SIGNATURES = {"og_%s_shape": (r"int depth, uint64_t shape\[3\]", 2), "og_%s_r1cs": (r"og_ctx\* ctx, int depth, og_r1cs\*\* out", 3),
              "og_%s_witness_d": (r"og_ctx\* ctx, int depth, const uint8_t\* inputs_d, size_t n, uint8_t\* witness_out_d", 5),
              "og_%s_prove_batch_d": (r"og_ctx\* ctx, const og_pk\* pk, int depth, const uint8_t\* inputs_d, size_t n, const uint8_t\* rs,\s+"
                                      r"uint8_t\* proofs_out, uint8_t\* public_out", 8)}
SHAPES = {"send": (5, {1: (8459, 8590), 2: (9192, 9322), 32: (31182, 31282)}),
          "redeem": (7, {1: (7000, 7131), 2: (7733, 7863), 32: (29723, 29823)})}


def _spec(statement):
    from tests import redeem_spec, send_spec
    return send_spec if statement == "send" else redeem_spec


def test_the_eight_symbols_are_declared_bound_and_exported():
    from owshen_amd import _abi, _lib, circuit
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so"))
    for statement in STATEMENTS:
        for pattern, (args, n_args) in SIGNATURES.items():
            name = pattern % statement
            assert re.search(r"^int %s\(%s\);" % (name, args), header, re.M), name
            assert name in _abi.SIGNATURES and _abi.SIGNATURES[name][0] is C.c_int
            assert getattr(_lib.lib, name).argtypes == _abi.SIGNATURES[name][1] and len(_abi.SIGNATURES[name][1]) == n_args
            assert hasattr(hooks, name), name
            twin = "og_claim_" + name[len("og_" + statement + "_"):]      # the conventions are those of the claim calls
            assert _abi.SIGNATURES[name] == _abi.SIGNATURES[twin], name
        for f in ("%s_shape", "%s_r1cs", "%s_r1cs_native", "pack_%s_inputs", "%s_witness", "%s_prove"):
            assert hasattr(circuit, f % statement), f % statement
    assert hasattr(circuit, "send_leaves") and hasattr(circuit, "redeem_change_leaf")


def test_the_header_states_both_statements():
    header = open(os.path.join(ROOT, "include", "owshen_gpu.h")).read()
    for word in ("n_wires = 1886 + 3 depth + (8 + depth) 730", "n_constraints = 2018 + 2 depth + (8 + depth) 730",
                 "n_wires = 1887 + 3 depth + (6 + depth) 730", "n_constraints = 2019 + 2 depth + (6 + depth) 730",
                 "x | amount | token | chain_id | pay_commitment | pay_amount | change_commitment | index (u64, low bytes) | siblings[depth]",
                 "x | amount | recipient | amount_out | token | chain_id | change_commitment | index (u64, low bytes) | siblings[depth]",
                 "field 5 if pay_amount >= 2^128", "field 3 if amount_out >= 2^128", "field 0 if x >= l", "field 7 if the index does not fit the tree",
                 "root, nullifier_hash, chain_id, pay_leaf, change_leaf", "root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf",
                 "claim, send and redeem publish the SAME nullifier_hash", "append pay_leaf, then", "pay amount_out of",
                 "Out of scope: a wave-wide walk"):
        assert word in header, word
    # the three owned statements state the one nullifier hash
    assert header.count("nullifier_hash = H(x, 1)") >= 3


@pytest.mark.parametrize("statement", STATEMENTS)
def test_shape_query_without_a_device(statement):
    from owshen_amd import _lib, circuit
    spec = _spec(statement)
    n_pub, want = SHAPES[statement]
    query = getattr(_lib.lib, f"og_{statement}_shape")
    shp = (C.c_uint64 * 3)()
    for depth in (1, 2, 32, 64):
        assert query(depth, shp) == 0
        assert (int(shp[0]), int(shp[1])) == spec.shape(depth) == getattr(circuit, statement + "_shape")(depth)
        assert int(shp[2]) == n_pub == spec.N_PUB
        assert depth not in want or spec.shape(depth) == want[depth]
    assert spec.shape(32)[1] + n_pub + 1 <= 1 << 15, "the depth-32 statement leaves the 2^15 domain"
    for depth in (0, 65, -1):
        assert query(depth, shp) == -1
    assert query(32, None) == -1


@pytest.mark.parametrize("statement", STATEMENTS)
def test_null_handles_are_refused_before_the_device(statement):
    from owshen_amd import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 512)()
    null = C.c_void_p()
    assert getattr(lib, f"og_{statement}_witness_d")(null, 2, buf, 1, buf) == -1 and b"null og_ctx" in lib.og_last_error()
    assert getattr(lib, f"og_{statement}_prove_batch_d")(null, null, 2, buf, 1, buf, buf, None) == -1
    assert getattr(lib, f"og_{statement}_r1cs")(null, 2, None) == -1


def test_the_python_builders_import_nothing_from_the_oracle():
    src = open(os.path.join(ROOT, "owshen_amd", "circuit.py")).read()
    assert "oracle" not in "".join(line for line in src.splitlines() if line.lstrip().startswith(("import ", "from ")))
