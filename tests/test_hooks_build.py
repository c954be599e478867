"""The shipped library carries no test hooks.

`libowshen_gpu.so` reads exactly two environment variables -- OG_SUB_BATCH (an operator's memory knob) and OG_DEBUG_SYNC
(fault bisection) -- and NONE of the ~50 A/B / test switches rounds 1-4 grew: not the launch-shape overrides, not the
thresholds that make rare paths reachable at toy sizes, not OG_MULTI_FAIL (which makes a multi-device call fail on purpose).
Those exist only in `libowshen_gpu_hooks.so` (-DOG_AB_HOOKS), which the hook-dependent tests load explicitly.  The reference
has no feature flags at all (/root/reference/Cargo.toml:1-54), and a node process inherits its environment."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "owshen_amd")
ALLOWED = {"OG_SUB_BATCH", "OG_DEBUG_SYNC"}


def _og_strings(path):
    out = subprocess.run(["strings", "-n", "4", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bOG_[A-Z][A-Z0-9_]+\b", out))


def test_default_library_names_only_two_environment_variables():
    names = _og_strings(os.path.join(PKG, "libowshen_gpu.so"))
    assert names <= ALLOWED, f"the shipped library mentions hook variables: {sorted(names - ALLOWED)}"
    assert names == ALLOWED


def test_hooks_library_has_the_switches_and_the_same_abi():
    import ctypes as C
    from owshen_amd import _lib
    from tests.test_abi import _header_symbols
    path = os.path.join(PKG, "libowshen_gpu_hooks.so")
    names = _og_strings(path)
    for must in ("OG_MULTI_FAIL", "OG_PIPE_MIN", "OG_ACC_WAVES_G1", "OG_G2_AFFINE", "OG_HEAVY", "OG_SUB_PLAN", "OG_GLV", "OG_SUB_BATCH"):
        assert must in names, must
    lib = C.CDLL(path)
    for s in _header_symbols():
        assert hasattr(lib, s), f"{s} missing from the hooks build"
    assert set(_lib.SIGNATURES) == set(_header_symbols())
    # the test seams exist in the hooks build only: the shipped library's exported set is the header's and nothing else
    shipped = C.CDLL(os.path.join(PKG, "libowshen_gpu.so"))
    for seam in ("og_hook_verify_miller_d", "og_hook_final_exp_d", "og_hook_fe_raw_d", "og_hook_ec_chain_d", "og_hook_w9_raw_d", "og_hook_w9_ec_chain_d"):
        assert hasattr(lib, seam), f"{seam} missing from the hooks build"
        assert not hasattr(shipped, seam), f"{seam} is in the shipped library"


def test_sources_read_the_environment_only_through_the_hook_macros():
    """every getenv in the product sources is one of the two allowed reads or lives inside the OG_AB_HOOKS block of ctx.h"""
    csrc = os.path.join(PKG, "csrc")
    hits = []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h", ".cpp", ".inc")):
            continue
        for no, line in enumerate(open(os.path.join(csrc, fn), errors="replace"), 1):
            code = line.split("//")[0]
            if "getenv" in code:
                hits.append((fn, no, code.strip()))
    allowed = [h for h in hits if any(f'getenv("{v}")' in h[2] for v in ALLOWED)]
    inside_hooks = [h for h in hits if h[0] == "ctx.h" and "getenv(name)" in h[2]]
    assert sorted(hits) == sorted(allowed + inside_hooks), [h for h in hits if h not in allowed and h not in inside_hooks]
    assert len(allowed) == 2 and len(inside_hooks) == 3
    # and the rejected kernel variants are not even compiled into the default library
    syms = subprocess.run(["strings", os.path.join(PKG, "libowshen_gpu.so")], capture_output=True, text=True).stdout
    for gone in ("k_accumulate_affine", "k_affine_meta"):
        assert gone not in syms, gone
