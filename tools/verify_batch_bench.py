#!/usr/bin/env python3
"""Times og_verify_batch_d against og_verify on one box, in one process, and writes profiles/verify_batch.json.

On one GPU: proves n in {1, 64, 1024, 4096} natural depth-32 withdraw statements and 8192 deposit statements once, corrupts every
eighth proof (so the batch has rejects: they leave the pipeline early, as in production), then times og_verify_batch_d alone --
proofs and public inputs device-resident, the copy of the flags included -- as the median of --reps calls after --warmup calls,
and og_vk_load once.  The yardstick is og_verify over the SAME proofs through a 16-thread pool (the host-only library; ctypes
releases the GIL), measured in the same run.  Acceptance (ISSUE "Measurement"): at n = 4096 natural proofs the GPU call beats
the pool by at least 2 x; the script exits 1 if it does not.

    python tools/verify_batch_bench.py [--reps 10] [--warmup 2] [--cpu-sample 8192] [--out profiles/verify_batch.json]
    python tools/verify_batch_bench.py --trace-child       # what `rocprofv3 --kernel-trace --stats -- python tools/... ` runs

The per-kernel breakdown comes from ONE separate run under `rocprofv3 --kernel-trace --stats` (the program after `--`, no counters),
started by this script as a fresh child process unless --no-trace."""
import argparse
import csv
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

README_RATES = {"natural_prove_per_s": 5155, "deposit_prove_per_s": 46164}


def _corrupt(proofs, pub, rnd):
    n = proofs.shape[0]
    for k, i in enumerate(range(0, n, 8)):
        if n < 8:
            break
        c = k % 3
        if c == 0:
            proofs[i, rnd.randrange(256)] ^= 1 << rnd.randrange(8)
        elif c == 1:
            pub[i] = pub[(i + 1) % n]
        else:
            proofs[i, 192:256] = 0
    return proofs, pub


def make_sets(ctx, sizes, n_deposit):
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    sets = {}
    depth = 32
    r1 = circuit.withdraw_r1cs(ctx.mimc7_constants(), depth, 0, 0)
    blob, vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    n_max = max(sizes)
    packed = np.stack([circuit.pack_inputs(rnd.randrange(fields.R), rnd.randrange(fields.R), rnd.randrange(1 << 64), rnd.randrange(1 << 160),
                                           rnd.randrange(fields.R), rnd.randrange(1 << depth), [rnd.randrange(fields.R) for _ in range(depth)],
                                           token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32)) for _ in range(n_max)])
    rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in range(n_max)]
    t0 = time.perf_counter()
    proofs, pub = circuit.prove_from_inputs(ctx, pk, depth, ctx.to_device(packed), rs, return_public=True)
    prove_s = time.perf_counter() - t0
    pk.close()
    ctx.release_scratch()
    vkb = g16.vk_to_bytes(vk)
    for n in sizes:
        p, q = _corrupt(proofs[:n].copy(), pub[:n].copy(), rnd)
        sets["natural_%d" % n] = (vkb, p, q)
    sets["_natural_prove_s"] = prove_s
    if n_deposit:
        r1 = circuit.deposit_r1cs(ctx.mimc7_constants())
        blob, vk = g16.setup(ctx, r1, 41, 42, 43, 44, 45)
        pk = g16.ProvingKey(ctx, blob)
        recs = np.stack([circuit.pack_deposit_inputs(rnd.randrange(fields.R), rnd.randrange(fields.R), rnd.randrange(1 << 160)) for _ in range(n_deposit)])
        rs = [(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in range(n_deposit)]
        proofs, pub = circuit.deposit_prove(ctx, pk, ctx.to_device(recs), rs, return_public=True)
        pk.close()
        ctx.release_scratch()
        p, q = _corrupt(proofs.copy(), pub.copy(), rnd)
        sets["deposit_%d" % n_deposit] = (g16.vk_to_bytes(vk), p, q)
    return sets


def cpu_pool(vkb, proofs, pub, idx, threads=16):
    """og_verify (host-only library) over proofs[idx] through a thread pool: (seconds, answers)"""
    from owshen_amd import api, verify_only
    items = [(api.bytes_to_ints(pub[i]), proofs[i].tobytes()) for i in idx]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        ans = list(ex.map(lambda e: bool(verify_only.verify(vkb, e[0], e[1])), items))
    return time.perf_counter() - t0, ans


def run(args):
    from owshen_amd import api, groth16 as g16, verify_only
    ctx = api.Context(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    sets = make_sets(ctx, sizes, args.deposit)
    out = {"tool": "tools/verify_batch_bench.py", "reps": args.reps, "warmup": args.warmup, "measured_on_gpu": True,
           "natural_prove_s_for_%d" % max(sizes): round(sets.pop("_natural_prove_s"), 3), "sets": {}, "readme_rates": README_RATES}
    tele = None
    try:
        import torch
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.02).start()
    except Exception as e:   # the helper is optional
        out["telemetry_error"] = repr(e)[:200]
    for name, (vkb, proofs, pub) in sets.items():
        n = proofs.shape[0]
        t0 = time.perf_counter()
        key = g16.VerifyingKey(ctx, vkb)
        load_ms = (time.perf_counter() - t0) * 1e3
        proofs_d, pub_d = ctx.to_device(proofs), ctx.to_device(pub)
        for _ in range(args.warmup):
            got = key.verify_batch(pub_d, proofs_d)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = key.verify_batch(pub_d, proofs_d)
            times.append((time.perf_counter() - t0) * 1e3)
        key.close()
        if args.trace_child:
            continue
        # the yardstick: all proofs when the set is small, else an evenly spaced sample scaled up (said so in the output)
        idx = list(range(n)) if n <= args.cpu_sample else list(range(0, n, n // args.cpu_sample))[:args.cpu_sample]
        cpu_s, ans = cpu_pool(vkb, proofs, pub, idx)
        assert [bool(got[i]) for i in idx] == ans, "og_verify_batch_d and og_verify disagree in %s" % name
        cpu_ms_full = cpu_s * 1e3 * n / len(idx)
        one_s, _ = cpu_pool(vkb, proofs, pub, [1 % n], threads=1)
        med = statistics.median(times)
        out["sets"][name] = {
            "n": n, "accepted": int(got.sum()), "vk_load_ms": round(load_ms, 2),
            "gpu_ms_min_median_max": [round(min(times), 3), round(med, 3), round(max(times), 3)],
            "gpu_proofs_per_s": round(n / med * 1e3, 1),
            "cpu16_ms": round(cpu_ms_full, 1), "cpu16_proofs_per_s": round(n / cpu_ms_full * 1e3, 1),
            "cpu16_measured_on": len(idx), "cpu16_extrapolated": len(idx) != n,
            "og_verify_one_proof_ms": round(one_s * 1e3, 2),
            "speedup_vs_cpu16": round(cpu_ms_full / med, 2),
        }
        print(name, json.dumps(out["sets"][name]), flush=True)
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    ctx.close()
    return out


def kernel_trace(args):
    """one separate run under rocprofv3 --kernel-trace --stats (kernel tracing only; the program after `--`)"""
    tmp = tempfile.mkdtemp(prefix="vfy_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "vfy", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", "--sizes", "4096", "--deposit", "0", "--reps", "3", "--warmup", "1"]
    try:
        subprocess.run(cmd, check=True, timeout=420, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    except Exception as e:
        return {"error": repr(e)[:300]}
    rows = []
    for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_vfy" in r.get("Name", ""):
                rows.append({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                             "avg_ms": round(float(r["AverageNs"]) / 1e6, 3)})
    return {"n": 4096, "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096")
    ap.add_argument("--deposit", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-sample", type=int, default=8192, help="og_verify runs on at most this many proofs of a set (evenly spaced) and is scaled to the set")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    out = run(args)
    if args.trace_child:
        return 0
    if not args.no_trace:
        out["kernel_trace"] = kernel_trace(args)
    gate = out["sets"].get("natural_4096")
    if gate:
        out["acceptance"] = {"rule": "gpu call at n = 4096 natural proofs at least 2 x the 16-thread og_verify pool of the same run",
                             "speedup": gate["speedup_vs_cpu16"], "met": gate["speedup_vs_cpu16"] >= 2.0}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out.get("acceptance")))
    return 0 if not gate or out["acceptance"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
