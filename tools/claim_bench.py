#!/usr/bin/env python3
"""Times og_claim_prove_batch_d beside og_transfer_prove_batch_d, the two witness calls alone, and og_note_scan_owned_batch_d beside
og_note_scan_batch_d, on one GPU, in one process, and writes profiles/claim.json.

Both statements at depth 32, records device-resident, the median of --reps calls after --warmup calls; engine clock and socket power
sampled on the host while the run lasts (bench.py GpuTelemetry).  The yardstick is `transfer` (and the ordinary scan) in the SAME run,
never `claim` itself and never a number from another day:
 (a) --n requests per call (default 4 096): claim beside transfer, and one profiled call's stage times (og_profile) for each;
 (b) the witness call alone for 1 and for --n requests, through the hooks build with OG_WITNESS_W9=0, so that transfer walks
     lane-local too (claim has no other walk): like for like.  The product count predicts, per request, 251 additions of ~12
     products plus ~750 for the inversion pass beside 37 hashes of 728 products for claim (~30 700), and 40 hashes for transfer
     (~29 100): a ratio near 1.05.  A ratio clearly above that is a finding to explain;
 (c) the scans at --memos memos (default 65 536), one memo in 1 024 the scanner's: the owned scan runs, for a hit, the reduction, 64
     table additions, an inversion and five permutations where the ordinary one runs ten permutations.
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/claim_bench.py [--n 4096] [--memos 65536] [--reps 5] [--warmup 1] [--out profiles/claim.json]"""
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
STATEMENTS = ("transfer", "claim")
ONE_IN = 1024
ELL = 2736030358979909402780800718157159386076813972158567259200215660948447373041


def _records(circuit, statement, n, rnd):
    from owshen_amd.api import FR_MODULUS as R
    recs = []
    for _ in range(n):
        amount = rnd.randrange(1, 1 << 64)
        common = dict(amount=amount, index=rnd.randrange(1 << DEPTH), siblings=[rnd.randrange(R) for _ in range(DEPTH)],
                      token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32))
        if statement == "transfer":
            recs.append(circuit.pack_transfer_inputs(nullifier=rnd.randrange(R), secret=rnd.randrange(R), pay_commitment=rnd.randrange(R),
                                                     pay_amount=rnd.randrange(amount + 1), change_commitment=rnd.randrange(R), **common))
        else:
            recs.append(circuit.pack_claim_inputs(x=rnd.randrange(ELL), out_commitment=rnd.randrange(R), **common))
    return np.stack(recs)


def _timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def _mmm(times, digits=3):
    return [round(min(times), digits), round(statistics.median(times), digits), round(max(times), digits)]


def measure(ctx, hctx, statement, args):
    from owshen_amd.api import FR_MODULUS as R
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    r1 = getattr(circuit, statement + "_r1cs")(ctx.mimc7_constants(), DEPTH)
    blob, vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    recs_d = ctx.to_device(_records(circuit, statement, args.n, rnd))
    rs = np.frombuffer(b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(2 * args.n)), dtype=np.uint8).reshape(args.n, 64).copy()
    prove = lambda c, k, d, r, **kw: getattr(circuit, statement + "_prove")(c, k, DEPTH, d, r, **kw)  # noqa: E731
    witness = lambda c, d: getattr(circuit, statement + "_witness")(c, DEPTH, d)  # noqa: E731
    out = {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d, "n": args.n}
    one_d, one_rs = recs_d[:1].contiguous(), rs[:1]
    out["one_request_ms_min_median_max"] = _mmm(_timed(lambda: prove(ctx, pk, one_d, one_rs), args.reps, args.warmup))
    batch = _timed(lambda: prove(ctx, pk, recs_d, rs), args.reps, args.warmup)
    ctx.profile(True)
    proofs, pub = prove(ctx, pk, recs_d, rs, return_public=True)
    stages = {k: [round(v[0], 3), v[1]] for k, v in ctx.profile_read().items() if v[1]}
    ctx.profile(False)
    vkb = g16.vk_to_bytes(vk)
    accepted = all(g16.verify(vkb, pub[i], proofs[i].tobytes()) for i in (0, args.n // 2, args.n - 1))
    out.update({"call_ms_min_median_max": _mmm(batch, 2), "proofs_per_s": round(args.n / statistics.median(batch) * 1e3, 1),
                "sampled_proofs_verify": bool(accepted), "stage_ms_and_launches_of_one_profiled_call": stages})
    del proofs, pub
    pk.close()
    ctx.release_scratch()
    # (b) the witness call alone, lane-local for both statements (the hooks build reads OG_WITNESS_W9)
    os.environ["OG_WITNESS_W9"] = "0"
    try:
        out["lane_local_witness_ms_min_median_max"] = {"1": _mmm(_timed(lambda: witness(hctx, one_d), args.reps, args.warmup)),
                                                       str(args.n): _mmm(_timed(lambda: witness(hctx, recs_d), args.reps, args.warmup))}
    finally:
        os.environ.pop("OG_WITNESS_W9", None)
    hctx.release_scratch()
    return out


def measure_scans(ctx, args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from note_scan_bench import _keys, seal_requests   # the ordinary scan's memos: one in 1 024 to the scanning key
    n = args.memos
    sks, pks = _keys(ctx, 1)
    req_d = ctx.to_device(seal_requests(pks, n, 4))
    want = np.zeros(n, dtype=np.uint32)
    want[::ONE_IN] = 1
    out = {"n": n, "hits": int(want.sum())}
    for name, seal, scan in (("ordinary", ctx.note_seal, ctx.note_scan), ("owned", ctx.note_seal_owned, ctx.note_scan_owned)):
        memos_d, notes_d, ok = seal(req_d)
        assert ok.all(), "a seeded seal request was refused"
        leaves_d = notes_d[:, 1, :].contiguous()
        assert np.array_equal(scan(sks[0], memos_d, leaves_d)[1], want), name
        assert not scan(sks[2], memos_d, leaves_d)[1].any()
        out[name] = {"scan_ms_min_median_max": _mmm(_timed(lambda: scan(sks[0], memos_d, leaves_d), args.reps, args.warmup)),
                     "scan_no_hits_ms_min_median_max": _mmm(_timed(lambda: scan(sks[2], memos_d, leaves_d), args.reps, args.warmup)),
                     "seal_ms_min_median_max": _mmm(_timed(lambda: seal(req_d), args.reps, args.warmup))}
        del memos_d, notes_d, leaves_d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--memos", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "claim.json"))
    args = ap.parse_args()
    import torch
    from owshen_amd import api, _lib
    from owshen_amd._abi import bind

    hooks = bind(C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so")))

    class HooksContext(api.Context):
        _lib = hooks

    ctx, hctx = api.Context(0), HooksContext(0)
    out = {"tool": "tools/claim_bench.py", "depth": DEPTH, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "yardstick": "og_transfer_prove_batch_d / og_transfer_witness_d / og_note_scan_batch_d in the same run"}
    tele = None
    try:
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.05).start()
    except Exception as e:  # (the numbers stand without it)
        out["telemetry_error"] = repr(e)[:200]
    for statement in STATEMENTS:
        out[statement] = measure(ctx, hctx, statement, args)
        print(statement, json.dumps(out[statement]), flush=True)
    out["scans"] = measure_scans(ctx, args)
    print("scans", json.dumps(out["scans"]), flush=True)
    hctx.close()
    ctx.close()
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    t, c, s = out["transfer"], out["claim"], out["scans"]
    wit = lambda d, k: d["lane_local_witness_ms_min_median_max"][k][1]  # noqa: E731
    products = {"claim": 251 * 12 + 750 + 37 * 728, "transfer": 40 * 728}
    out["ratios"] = {
        "claim_over_transfer_proofs_per_s": round(c["proofs_per_s"] / t["proofs_per_s"], 4),
        "claim_over_transfer_wires": round(c["n_wires"] / t["n_wires"], 4),
        "one_request_ms_claim_over_transfer": round(c["one_request_ms_min_median_max"][1] / t["one_request_ms_min_median_max"][1], 4),
        "lane_local_witness_ms_claim_over_transfer": {k: round(wit(c, k) / wit(t, k), 4) for k in c["lane_local_witness_ms_min_median_max"]},
        "predicted_products_per_request": products,
        "predicted_witness_ratio": round(products["claim"] / products["transfer"], 4),
        "scan_owned_over_scan": round(s["owned"]["scan_ms_min_median_max"][1] / s["ordinary"]["scan_ms_min_median_max"][1], 4),
        "scan_owned_over_scan_no_hits": round(s["owned"]["scan_no_hits_ms_min_median_max"][1] / s["ordinary"]["scan_no_hits_ms_min_median_max"][1], 4),
        "seal_owned_over_seal": round(s["owned"]["seal_ms_min_median_max"][1] / s["ordinary"]["seal_ms_min_median_max"][1], 4),
        "note": "one request of the SHIPPED library: transfer walks wave-wide (calls of at most 512 requests), claim has the lane-local "
                "walk only -- that ratio is the price of the missing wave-wide form, not of the multiplication",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["ratios"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
