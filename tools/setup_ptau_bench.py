"""og_setup_ptau / og_pk_contribute at the benchmark key (dense withdraw circuit, 2^18 wires, domain 2^17) beside og_setup at the
same shape in the same process; recorded, not gated (load-time work).  The power-17 .ptau is made here, on the GPU, from a known
(tau, alpha, beta), so the ceremony key can be compared with og_setup's byte for byte.
usage: python tools/setup_ptau_bench.py [--out profiles/setup_ptau.json] [--depth 32]"""
import argparse
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from owshen_amd import api, circuit, groth16 as g16, ptau   # noqa: E402

from tests.ptau_cases import make_ptau   # noqa: E402  (the tests' .ptau writer: points by og_scalar_mul_d, the encoding in Python)


class PeakSampler:
    """free device bytes (og_mem_info through a second context: calls on one context are serialised) sampled while a call runs"""

    def __init__(self):
        self.ctx = api.Context(0)
        self.low = None

    def run(self, fn):
        before = self.ctx.mem_info()["device_free_bytes"]
        self.low, stop = before, threading.Event()

        def loop():
            while not stop.is_set():
                self.low = min(self.low, self.ctx.mem_info()["device_free_bytes"])
                time.sleep(0.005)
        th = threading.Thread(target=loop)
        th.start()
        t0 = time.perf_counter()
        try:
            res = fn()
        finally:
            dt = time.perf_counter() - t0
            stop.set()
            th.join()
        return res, dt, before - self.low


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--depth", type=int, default=32)
    a = ap.parse_args()
    ctx = api.Context(0)
    n_pad3, n_pad2 = circuit.baseline_shape(a.depth, dense=True)
    r1 = circuit.withdraw_r1cs(ctx.mimc7_constants(), a.depth, n_pad3, n_pad2, dense=True)
    tau, alpha, beta, delta = 0x7654321, 0x2345678, 0x3456789, 0x56789AB
    t0 = time.perf_counter()
    data = make_ptau(ctx, r1.log_d, tau, alpha, beta)
    t_file = time.perf_counter() - t0
    ctx.release_scratch()
    sampler = PeakSampler()
    out = {"n_wires": r1.n_wires, "domain": r1.domain_size, "nnz": [int(m.nnz) for m in (r1.a, r1.b, r1.c)], "ptau_bytes": len(data),
           "ptau_made_s": round(t_file, 3), "runs": []}
    for _rep in range(2):
        (pk, vk), t_ptau, peak_ptau = sampler.run(lambda: ptau.setup(ctx, r1, data))
        (pk_c, vk_c), t_con, peak_con = sampler.run(lambda: ptau.contribute(ctx, pk, vk, delta))
        (want, want_vk), t_setup, peak_setup = sampler.run(lambda: g16.setup(ctx, r1, tau, alpha, beta, 1, 1))
        out["runs"].append({"setup_ptau_s": round(t_ptau, 3), "pk_contribute_s": round(t_con, 3), "og_setup_s": round(t_setup, 3),
                            "setup_ptau_peak_device_bytes": int(peak_ptau), "pk_contribute_peak_device_bytes": int(peak_con),
                            "og_setup_peak_device_bytes": int(peak_setup)})
    out["byte_identical"] = bool(pk == want and vk == g16.vk_to_bytes(want_vk))
    want_c, want_vk_c = g16.setup(ctx, r1, tau, alpha, beta, 1, delta)
    out["contributed_byte_identical"] = bool(pk_c == want_c and vk_c == g16.vk_to_bytes(want_vk_c))
    out["pk_bytes"] = len(pk)
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
