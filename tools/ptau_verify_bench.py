"""og_ptau_verify / og_pk_verify at the benchmark key (dense withdraw circuit, 2^18 wires, domain 2^17, a power-17 .ptau made from a
known tau as tools/setup_ptau_bench.py makes it) beside og_setup_ptau in the same process: wall time, best of three after one warm
call, and the peak device memory of each; recorded, not gated (load-time work).  og_pk_verify contains a whole og_setup_ptau, so
`pk_verify_minus_setup_s` is what its sums and pairings cost.
usage: python tools/ptau_verify_bench.py [--out profiles/ptau_verify.json] [--depth 32]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from owshen_amd import api, circuit, ptau   # noqa: E402

from tests.ptau_cases import make_ptau   # noqa: E402  (the tests' .ptau writer: points by og_scalar_mul_d, the encoding in Python)
from tools.setup_ptau_bench import PeakSampler   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--depth", type=int, default=32)
    a = ap.parse_args()
    ctx = api.Context(0)
    n_pad3, n_pad2 = circuit.baseline_shape(a.depth, dense=True)
    r1 = circuit.withdraw_r1cs(ctx.mimc7_constants(), a.depth, n_pad3, n_pad2, dense=True)
    tau, alpha, beta, delta = 0x7654321, 0x2345678, 0x3456789, 0x56789AB
    data = make_ptau(ctx, r1.log_d, tau, alpha, beta)
    pk, vk = ptau.contribute(ctx, *ptau.setup(ctx, r1, data), delta)
    ctx.release_scratch()
    sampler = PeakSampler()
    calls = {"ptau_verify": lambda: ptau.verify_mask(ctx, data), "pk_verify": lambda: ptau.verify_key_mask(ctx, r1, data, pk, vk),
             "setup_ptau": lambda: len(ptau.setup(ctx, r1, data)[0])}
    out = {"n_wires": r1.n_wires, "domain": r1.domain_size, "ptau_bytes": len(data), "pk_bytes": len(pk), "repeats": 3}
    for name, fn in calls.items():
        res = fn()                                              # the warm call
        runs = [sampler.run(fn) for _ in range(3)]
        out[name + "_s"] = round(min(r[1] for r in runs), 3)
        out[name + "_runs_s"] = [round(r[1], 3) for r in runs]
        out[name + "_peak_device_bytes"] = int(max(r[2] for r in runs))
        if name != "setup_ptau":
            out[name + "_mask"] = int(res)
    out["pk_verify_minus_setup_s"] = round(out["pk_verify_s"] - out["setup_ptau_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sampler.ctx.close()
    ctx.close()


if __name__ == "__main__":
    main()
