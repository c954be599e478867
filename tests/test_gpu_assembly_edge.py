"""GPU: the proof assembly at the edges of the blinding pair (r, s) -- every scalar of tests/assembly_edge_cases.py as r, as s and as
r s, in every form of the assembly (a wave, a lane per GLV half or a lane per 254-bit scalar; two parts with the G2 tree or one part
with a lane per proof; the host), under a key with random toxic values and under the two keys whose bases and proof elements are the
point at infinity; byte for byte the C restatement, whose K0 proofs the verifier accepts.  The hooks build: the forms are switched
through its environment; tests/test_emu_assembly_edge.py confirms on the interpreter which kernels each switch launches."""
import pytest

from tests import assembly_edge_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(ctx_hooks):
    w = cases.world(ctx_hooks)
    yield w
    w.close()


def test_gpu_assembly_edge_coverage(ctx_hooks, world):
    assert len(world.pairs) >= 7 + 3 * len(cases.SCALARS)
    assert all(v >= 1 for v in world.cover.values())
    cases.infinity_checks(ctx_hooks)


def test_gpu_assembly_edge_every_k0_proof_verifies(world):
    assert world.verify_k0(world.pairs, batched=True) == len(world.pairs)


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_gpu_assembly_edge_forms(ctx_hooks, world, monkeypatch, form):
    n, calls = cases.run_form(ctx_hooks, monkeypatch, form, "K0", world.pairs, check_py=12 if form == "w9/two-part" else 0)
    print(f"assembly_edge K0 {form}: {n} proofs in {calls} calls")
    assert n == len(world.pairs)


@pytest.mark.parametrize("key", ["Ka", "Kb"])
@pytest.mark.parametrize("form", list(cases.FORMS))
def test_gpu_assembly_edge_infinite_bases(ctx_hooks, world, monkeypatch, form, key):
    pairs = cases.edge_key_pairs(world.pairs)
    n, calls = cases.run_form(ctx_hooks, monkeypatch, form, key, pairs, check_py=len(pairs) if form == "w9/two-part" else 0)
    print(f"assembly_edge {key} {form}: {n} proofs in {calls} calls")
    assert n >= len(pairs) >= 12


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_gpu_assembly_noncanonical_pairs_prove_as_their_residues(ctx_hooks, world, monkeypatch, form):
    n, _calls = cases.run_form(ctx_hooks, monkeypatch, form, "K0", cases.noncanonical_pairs(), noncanonical=True)
    assert n >= 7
