#!/usr/bin/env python3
"""Times og_send_prove_batch_d and og_redeem_prove_batch_d beside the statements they replace -- transfer, split and claim -- on one
GPU, in one process, and writes profiles/send_redeem.json.

All five statements at depth 32, records device-resident, the median of --reps repetitions after --warmup warm calls; inside every
repetition the five statements take turns, so that a drift of the clock falls on all of them alike; engine clock and socket power
sampled on the host while the run lasts (bench.py GpuTelemetry).  The yardsticks are the existing statements in the SAME run, never
the new code itself and never a number from another day:
 (a) --n requests per call (default 4 096): send beside transfer and beside claim, redeem beside split, and the figure the two
     statements exist for: one claim call plus one transfer call against one send call for the same number of notes, and
     claim + split against redeem;
 (b) the witness call alone for 1 and for --n requests, through the hooks build with OG_WITNESS_W9=0, so that transfer and split walk
     lane-local too (the owned statements have no other walk): like for like.  The product count predicts, per request, claim's
     251 additions of ~12 products, ~750 for the inversion pass and 37 hashes of 728 (~30 700); send has three hashes more and
     redeem one: 1.07 and 1.02 of claim.  A ratio more than a tenth above its prediction is a finding to explain;
 (c) one request through the shipped library, for all five.
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/send_redeem_bench.py [--n 4096] [--reps 5] [--warmup 1] [--out profiles/send_redeem.json]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

DEPTH = 32
STATEMENTS = ("transfer", "split", "claim", "send", "redeem")
ELL = 2736030358979909402780800718157159386076813972158567259200215660948447373041
HASHES = {"transfer": 40, "split": 38, "claim": 37, "send": 40, "redeem": 38}
OWNED = ("claim", "send", "redeem")


def _records(circuit, statement, n, rnd):
    from owshen_amd.api import FR_MODULUS as R
    recs = []
    for _ in range(n):
        amount = rnd.randrange(1, 1 << 64)
        f = lambda: rnd.randrange(R)  # noqa: E731
        common = dict(amount=amount, index=rnd.randrange(1 << DEPTH), siblings=[f() for _ in range(DEPTH)], token=rnd.randrange(1 << 160),
                      chain_id=rnd.randrange(1 << 32))
        part = rnd.randrange(amount + 1)
        if statement == "transfer":
            rec = circuit.pack_transfer_inputs(nullifier=f(), secret=f(), pay_commitment=f(), pay_amount=part, change_commitment=f(), **common)
        elif statement == "split":
            rec = circuit.pack_split_inputs(nullifier=f(), secret=f(), recipient=rnd.randrange(1 << 160), amount_out=part, change_commitment=f(),
                                            **common)
        elif statement == "claim":
            rec = circuit.pack_claim_inputs(x=rnd.randrange(ELL), out_commitment=f(), **common)
        elif statement == "send":
            rec = circuit.pack_send_inputs(x=rnd.randrange(ELL), pay_commitment=f(), pay_amount=part, change_commitment=f(), **common)
        else:
            rec = circuit.pack_redeem_inputs(x=rnd.randrange(ELL), recipient=rnd.randrange(1 << 160), amount_out=part, change_commitment=f(),
                                             **common)
        recs.append(rec)
    return np.stack(recs)


def _turns(calls, reps, warmup):
    """{name: [ms per repetition]}: in every repetition each call runs once, in the order given"""
    for _ in range(warmup):
        for call in calls.values():
            call()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def _mmm(times, digits=3):
    return [round(min(times), digits), round(statistics.median(times), digits), round(max(times), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "send_redeem.json"))
    args = ap.parse_args()
    import torch
    from owshen_amd import api, circuit, groth16 as g16, _lib
    from owshen_amd._abi import bind
    from owshen_amd.api import FR_MODULUS as R

    hooks = bind(C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so")))

    class HooksContext(api.Context):
        _lib = hooks

    ctx, hctx = api.Context(0), HooksContext(0)
    n = args.n
    out = {"tool": "tools/send_redeem_bench.py", "depth": DEPTH, "n": n, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "order_inside_a_repetition": list(STATEMENTS),
           "yardstick": "transfer, split and claim in the same run, taking turns with send and redeem inside every repetition"}
    tele = None
    try:
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.05).start()
    except Exception as e:  # (the numbers stand without it)
        out["telemetry_error"] = repr(e)[:200]
    rnd = random.Random(4096)
    rs = np.frombuffer(b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(2 * n)), dtype=np.uint8).reshape(n, 64).copy()
    keys, vks, recs, ones = {}, {}, {}, {}
    for s in STATEMENTS:
        r1 = getattr(circuit, s + "_r1cs")(ctx.mimc7_constants(), DEPTH)
        blob, vks[s] = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
        keys[s] = g16.ProvingKey(ctx, blob)
        recs[s] = ctx.to_device(_records(circuit, s, n, rnd))
        ones[s] = recs[s][:1].contiguous()
        out[s] = {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d}
    prove = lambda s, d, r, **kw: getattr(circuit, s + "_prove")(ctx, keys[s], DEPTH, d, r, **kw)  # noqa: E731
    witness = lambda s, d: getattr(circuit, s + "_witness")(hctx, DEPTH, d)  # noqa: E731
    # (c) one request, the shipped library; (a) n requests per call
    one = _turns({s: (lambda s=s: prove(s, ones[s], rs[:1])) for s in STATEMENTS}, args.reps, args.warmup)
    batch = _turns({s: (lambda s=s: prove(s, recs[s], rs)) for s in STATEMENTS}, args.reps, args.warmup)
    for s in STATEMENTS:
        proofs, pub = prove(s, recs[s], rs, return_public=True)
        vkb = g16.vk_to_bytes(vks[s])
        accepted = all(g16.verify(vkb, pub[i], proofs[i].tobytes()) for i in (0, n // 2, n - 1))
        out[s].update({"one_request_ms_min_median_max": _mmm(one[s]), "call_ms_min_median_max": _mmm(batch[s], 2),
                       "proofs_per_s": round(n / statistics.median(batch[s]) * 1e3, 1), "sampled_proofs_verify": bool(accepted)})
        del proofs, pub
        print(s, json.dumps(out[s]), flush=True)
    for s in STATEMENTS:
        keys[s].close()
    ctx.release_scratch()
    # (b) the witness call alone, lane-local for all five (the hooks build reads OG_WITNESS_W9)
    os.environ["OG_WITNESS_W9"] = "0"
    try:
        w1 = _turns({s: (lambda s=s: witness(s, ones[s])) for s in STATEMENTS}, args.reps, args.warmup)
        wn = _turns({s: (lambda s=s: witness(s, recs[s])) for s in STATEMENTS}, args.reps, args.warmup)
    finally:
        os.environ.pop("OG_WITNESS_W9", None)
    for s in STATEMENTS:
        out[s]["lane_local_witness_ms_min_median_max"] = {"1": _mmm(w1[s]), str(n): _mmm(wn[s])}
    hctx.close()
    ctx.close()
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    call = lambda s: out[s]["call_ms_min_median_max"][1]  # noqa: E731
    one_ms = lambda s: out[s]["one_request_ms_min_median_max"][1]  # noqa: E731
    wit = lambda s, k: out[s]["lane_local_witness_ms_min_median_max"][k][1]  # noqa: E731
    products = {s: HASHES[s] * 728 + (251 * 12 + 750 if s in OWNED else 0) for s in STATEMENTS}
    sizes = ("1", str(n))
    out["ratios"] = {
        "send_over_transfer_call_ms": round(call("send") / call("transfer"), 4),
        "send_over_claim_call_ms": round(call("send") / call("claim"), 4),
        "redeem_over_split_call_ms": round(call("redeem") / call("split"), 4),
        "claim_plus_transfer_over_send_call_ms": round((call("claim") + call("transfer")) / call("send"), 4),
        "claim_plus_split_over_redeem_call_ms": round((call("claim") + call("split")) / call("redeem"), 4),
        "one_request_claim_plus_transfer_over_send": round((one_ms("claim") + one_ms("transfer")) / one_ms("send"), 4),
        "one_request_claim_plus_split_over_redeem": round((one_ms("claim") + one_ms("split")) / one_ms("redeem"), 4),
        "lane_local_witness_ms_send_over_claim": {k: round(wit("send", k) / wit("claim", k), 4) for k in sizes},
        "lane_local_witness_ms_redeem_over_claim": {k: round(wit("redeem", k) / wit("claim", k), 4) for k in sizes},
        "lane_local_witness_ms_send_over_transfer": {k: round(wit("send", k) / wit("transfer", k), 4) for k in sizes},
        "lane_local_witness_ms_redeem_over_split": {k: round(wit("redeem", k) / wit("split", k), 4) for k in sizes},
        "predicted_products_per_request": products,
        "predicted_witness_ratio_send_over_claim": round(products["send"] / products["claim"], 4),
        "predicted_witness_ratio_redeem_over_claim": round(products["redeem"] / products["claim"], 4),
        "note": "one request of the SHIPPED library: transfer and split walk wave-wide (calls of at most 512 requests), the owned "
                "statements have the lane-local walk only",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["ratios"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
