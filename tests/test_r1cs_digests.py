"""The R1CS of every statement with a Merkle walk, byte for byte: SHA-256 over n_wires | n_pub | ptr | col | val of A, B and C, for the
Python builder (owshen_amd/circuit.py) and the native one (keygen.hip, on the CPU interpreter), against tests/golden/r1cs_digests.json.

The digests are a recording (`python -m tests.test_r1cs_digests` writes them), made before the four builders were folded onto
shared gadgets: row order, wire allocation order and term order inside every linear combination decide key and proof bytes, and the
row-by-row comparisons against the specs would let a reordering through that both builders and a spec happen to share.  Depth 1 is
the walk whose first level is also the root level, depth 2 has one inner level and the root level; withdraw's padding case crosses
the 64-gate segment of the chained gates, with and without the density rows."""
import hashlib
import json
import os

import pytest

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r1cs_digests.json")
WITHDRAW = [(1, 0, 0, 0), (2, 0, 0, 0), (2, 2, 65, 0), (2, 2, 65, 1)]   # (depth, n_pad3, n_pad2, dense)
DEPTHS = (1, 2)


def digest(r1cs):
    h = hashlib.sha256()
    h.update(int(r1cs.n_wires).to_bytes(8, "little") + int(r1cs.n_pub).to_bytes(8, "little"))
    for m in (r1cs.a, r1cs.b, r1cs.c):
        for arr in (m.ptr, m.col, m.val):
            h.update(arr.tobytes())
    return h.hexdigest()


def cases(ctx):
    """name -> (python builder, native builder), each a thunk that returns an R1CS"""
    from owshen_amd import circuit
    consts = ctx.mimc7_constants()
    out = {}
    for d, p3, p2, dense in WITHDRAW:
        out[f"withdraw depth={d} n_pad3={p3} n_pad2={p2} dense={dense}"] = (
            lambda a=(d, p3, p2, bool(dense)): circuit.withdraw_r1cs(consts, *a),
            lambda a=(d, p3, p2, bool(dense)): circuit.withdraw_r1cs_native(ctx, *a))
    for st in ("split", "join", "transfer"):
        for d in DEPTHS:
            out[f"{st} depth={d}"] = (lambda st=st, d=d: getattr(circuit, st + "_r1cs")(consts, d),
                                      lambda st=st, d=d: getattr(circuit, st + "_r1cs_native")(ctx, d))
    return out


def compute(ctx):
    return {name: {"python": digest(py()), "native": digest(native())} for name, (py, native) in cases(ctx).items()}


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_r1cs_digests(ectx):
    with open(_GOLDEN) as f:
        want = json.load(f)
    got = compute(ectx)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
        assert got[name]["python"] == got[name]["native"], name   # (the two builders agreed when the digests were recorded)


if __name__ == "__main__":
    from tests import emu
    with open(_GOLDEN, "w") as f:
        json.dump(compute(emu.Ctx()), f, indent=1, sort_keys=True)
        f.write("\n")
