"""GPU: the quotient pipeline (h_poly, owshen_amd/csrc/ntt.hip) where only the CPU interpreter had taken it, and where nothing had:
* k_ntt_block4's lazy butterflies ("a value grows by <= 3N per stage", sums up to 36N subtracted through 40N, limbs up to 2^31 into
  fe_mul) on the inputs that maximise every intermediate sum, radix-4 == radix-2 == the C restatement -- the GPU twin of
  tests/test_emu_kernels.py::test_emu_quotient_radix4_equals_radix2_on_extreme_inputs (same triples: tests/quotient_cases.py);
* the stage-block shapes no test had run: a second block of 4 stages (2^14), a FULL 10-stage second block (2^20) and three
  blocks (2^21; a .zkey import makes every domain size reachable).
Host time of the C restatement's quotient (one thread) on the 8-core build container: 10.3 s at 2^20 and 21.5 s at 2^21, so the
expected coefficients come from quotient_cases.block_shape_oracle, which computes each size once per session.  On the MI355X host
the whole test, oracle included, took 3.2 s (2^20) and 7.8 s (2^21); the extreme-input case at 2^17 took 1.0 s."""
import pytest

from tests import quotient_cases as qc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log_d", [4, 10, 11, 12, 17])
def test_quotient_radix4_equals_radix2_on_extreme_inputs(ctx_hooks, log_d, monkeypatch):
    from oracle.c import binding as oc
    for k, (a, b, c) in enumerate(qc.extreme_triples(1 << log_d)):
        ad, bd, cd = (ctx_hooks.to_device(x) for x in (a, b, c))
        monkeypatch.delenv("OG_NTT_RADIX4", raising=False)
        r4 = ctx_hooks.to_host(ctx_hooks.h_poly(ad, bd, cd)).tobytes()
        monkeypatch.setenv("OG_NTT_RADIX4", "0")
        r2 = ctx_hooks.to_host(ctx_hooks.h_poly(ad, bd, cd)).tobytes()
        want = oc.h_poly(a, b, c).tobytes()
        assert r4 == want, (log_d, k, "radix-4")
        assert r2 == want, (log_d, k, "radix-2")


@pytest.mark.parametrize("log_d", [14, 20, 21])
def test_h_poly_block_shapes(ctx, log_d):
    """a second block of 4 stages, a full 10-stage second block, three blocks: random evaluations with 0 / 1 / r - 1 riding along"""
    a, b, c = qc.block_shape_inputs(log_d)
    got = ctx.to_host(ctx.h_poly(ctx.to_device(a), ctx.to_device(b), ctx.to_device(c)))
    assert got.tobytes() == qc.block_shape_oracle(log_d).tobytes()
