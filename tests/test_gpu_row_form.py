"""The A and B queries over the QAP rows on the GPU through the C ABI; cases in tests/row_form_cases.py, at toy size.  Plus ONE
full-size case: the dense 2^18-wire key, the only place where the 16-bit tables and the two-level digit sort meet the row map at
its real size (131 k rows)."""
import numpy as np
import pytest

from tests import row_form_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 5])
def test_row_form_proofs_are_the_plain_blobs_and_the_oracles(ctx, n):
    cases.case_same_proofs(ctx, n)


def test_row_form_through_the_stage_pipeline(ctx_hooks, monkeypatch):
    cases.case_same_proofs_pipelined(ctx_hooks, monkeypatch)


def test_row_form_with_the_host_assembly(ctx):
    cases.case_host_chains(ctx)


def test_rule_on_the_wide_keys(ctx):
    cases.case_rule_wide_keys(ctx)


def test_rule_keeps_the_natural_withdraw_key_on_the_wires(ctx):
    cases.case_rule_natural_withdraw(ctx)


def test_rule_decides_at_load_whatever_the_extension(ctx_hooks, monkeypatch):
    cases.case_rule_decides_at_load(ctx_hooks, monkeypatch)


def test_edge_scalars(ctx):
    cases.case_edge_scalars(ctx)


@pytest.mark.parametrize("name", cases.BAD)
def test_a_wrong_extension_is_refused(ctx, name):
    cases.case_refusal(ctx, name)


@pytest.mark.parametrize("world,n", [(2, 1), (2, 4), (3, 1), (3, 4)])
def test_window_sharded_front_in_row_form(ctx, world, n):
    cases.case_sharded(ctx, world, n)


def test_dense_full_size_key_in_row_form_gives_the_plain_blobs_bytes(ctx):
    """2 proofs of the dense 2^18-wire / 2^17-domain circuit: the key with its extension against the plain blob, and og_verify.
    (The plain blob at this size is pinned to the C restatement by test_gpu_fullsize_pipeline.py.)"""
    from owshen_amd import circuit, groth16 as g16
    from tests.test_gpu_fullsize_pipeline import _rand_fr, _records
    depth = 32
    n_pad3, n_pad2 = circuit.baseline_shape(depth, dense=True)
    r1 = circuit.withdraw_r1cs(ctx.mimc7_constants(), depth, n_pad3, n_pad2, dense=True)
    assert (r1.n_wires, r1.domain_size) == (1 << 18, 1 << 17)
    blob, vk = g16.setup(ctx, r1, 0x7654321, 0x2345678, 0x3456789, 0x456789A, 0x56789AB)
    assert blob.rows is not None and len(blob.rows) == 64 + r1.n_rows * 192
    row, plain = g16.ProvingKey(ctx, blob), g16.ProvingKey(ctx, bytes(blob))
    try:
        f = row.query_forms()
        assert [f[q]["form"] for q in ("a", "b1", "b2", "l", "h")] == ["row", "row", "row", "wire", "wire"], f
        assert f["a"]["table"] == f["b1"]["table"] == "a" and f["b2"]["table"] == "b2"
        assert 131000 <= f["a"]["points"] == f["b1"]["points"] == f["b2"]["points"] <= r1.n_rows and f["a"]["bits"] == 16, f
        assert row.density() == plain.density() and row.windows() == plain.windows()
        assert row.density()["a"] == row.density()["b"] == 1 << 18
        rng = np.random.default_rng(218)
        recs_d = ctx.to_device(_records(rng, 2, depth))
        rs = _rand_fr(rng, 2, 2).reshape(2, 64)
        got, pub = circuit.prove_from_inputs(ctx, row, depth, recs_d, rs, n_pad3, n_pad2, return_public=True)
        want = circuit.prove_from_inputs(ctx, plain, depth, recs_d, rs, n_pad3, n_pad2)
        assert got.tobytes() == want.tobytes()
        vkb = g16.vk_to_bytes(vk)
        assert all(g16.verify(vkb, pub[i], got[i].tobytes()) for i in range(2))
        assert not g16.verify(vkb, pub[1], got[0].tobytes())
    finally:
        row.close()
        plain.close()
        ctx.release_scratch()
