"""The proof assembly at the edges of (r, s) on the CPU interpreter: every form of tests/assembly_edge_cases.py (confirmed by the plan,
the timed regions AND the kernels the issue log names) on a reduced list that still covers every class of GLV halves in every
position, the two keys whose bases and proof elements are the point at infinity, and the non-canonical pairs;
tests/test_gpu_assembly_edge.py proves the whole list on the hardware."""
import pytest

from tests import assembly_edge_cases as cases

NONCANONICAL_FORMS = list(cases.FORMS)
EDGE_KEY_FORMS = ["w9/two-part", "w9/one-stream", "glv/two-part", "glv/one-part", "plain/two-part", "plain/one-part", "host"]


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    cases.world(c).close()
    c.close()


def test_the_pairs_cover_every_class_of_halves_the_library_forms(ectx):
    w = cases.world(ectx)
    assert len(w.pairs) >= 7 + 3 * len(cases.SCALARS) and len(cases.SCALARS) >= 60
    assert all(v >= 1 for v in w.cover.values()) and set(w.cover) == {(p, c) for p in cases.POSITIONS for c in cases.CLASSES}
    red = cases.reduced_pairs(ectx._lib, w.pairs)
    assert red[:7] == w.pairs[:7] and len(red) <= 16
    cases.infinity_checks(ectx)
    assert w.verify_k0(red, batched=False) == len(red)


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_emu_assembly_edge_forms(ectx, monkeypatch, tmp_path, form):
    w = cases.world(ectx)
    pairs = cases.reduced_pairs(ectx._lib, w.pairs)
    n, calls = cases.run_form(ectx, monkeypatch, form, "K0", pairs, issue_log=str(tmp_path / "issue.log"), check_py=12 if form == "glv/two-part" else 0)
    assert n >= len(pairs) and calls >= 1


@pytest.mark.parametrize("key", ["Ka", "Kb"])
@pytest.mark.parametrize("form", EDGE_KEY_FORMS)
def test_emu_assembly_edge_infinite_bases(ectx, monkeypatch, tmp_path, form, key):
    w = cases.world(ectx)
    n, _calls = cases.run_form(ectx, monkeypatch, form, key, w.pairs[:7], issue_log=str(tmp_path / "issue.log"), check_py=7 if form == "glv/two-part" else 0)
    assert n == 7


@pytest.mark.parametrize("form", NONCANONICAL_FORMS)
def test_emu_assembly_noncanonical_pairs_prove_as_their_residues(ectx, monkeypatch, tmp_path, form):
    n, _calls = cases.run_form(ectx, monkeypatch, form, "K0", cases.noncanonical_pairs(), issue_log=str(tmp_path / "issue.log"), noncanonical=True)
    assert n >= 7
