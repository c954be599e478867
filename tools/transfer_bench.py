#!/usr/bin/env python3
"""Times og_transfer_prove_batch_d beside og_split_prove_batch_d and og_withdraw_prove_batch_d on one GPU, in one process, and writes
profiles/transfer.json.

All three statements at depth 32 (the withdraw statement natural: padding 0 / 0), records device-resident, the median of --reps calls
after --warmup calls; engine clock and socket power sampled on the host while the run lasts (bench.py GpuTelemetry).  Every
yardstick is another call of the SAME run:
 (a) --n requests per call (default 4 096), transfer beside split, and one profiled call's stage times (og_profile) for each.
     split lost 5.3 % against withdraw for 6.5 % more wires; transfer carries 5.2 % more wires than split, so a ratio (transfer
     proofs/s over split proofs/s) below 0.90 is more than twice the added wires: a finding, to be explained from the stage times;
 (b) ONE request per call, for transfer, split and withdraw;
 (c) the witness call alone for 1 and for --n requests, og_transfer_witness_d against og_split_witness_d and og_withdraw_witness_d.
     For one request the wave-wide walk's dependent chain is withdraw's chain: a ratio above 1.25 to withdraw's witness call is a
     finding (the margin covers the wider first two launches and 12 % more wires to convert, not extra permutations on the chain);
 (d) one request with OG_WITNESS_W9=0 through the hooks build: what the wave-wide form bought.
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/transfer_bench.py [--n 4096] [--reps 5] [--warmup 1] [--out profiles/transfer.json]"""
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
STATEMENTS = ("withdraw", "split", "transfer")


def _records(circuit, statement, n, rnd):
    from oracle.py import fields
    recs = []
    for _ in range(n):
        amount = rnd.randrange(1, 1 << 64)
        common = dict(nullifier=rnd.randrange(fields.R), secret=rnd.randrange(fields.R), amount=amount, index=rnd.randrange(1 << DEPTH),
                      siblings=[rnd.randrange(fields.R) for _ in range(DEPTH)], token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32))
        if statement == "transfer":
            recs.append(circuit.pack_transfer_inputs(pay_commitment=rnd.randrange(fields.R), pay_amount=rnd.randrange(amount + 1),
                                                     change_commitment=rnd.randrange(fields.R), **common))
        elif statement == "split":
            recs.append(circuit.pack_split_inputs(recipient=rnd.randrange(1 << 160), amount_out=rnd.randrange(amount + 1),
                                                  change_commitment=rnd.randrange(fields.R), **common))
        else:
            recs.append(circuit.pack_inputs(recipient=rnd.randrange(1 << 160), pad_seed=0, **common))
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


def _mmm(times, digits):
    return [round(min(times), digits), round(statistics.median(times), digits), round(max(times), digits)]


def _calls(circuit, ctx, statement):
    """(prove(pk, records, rs, **kw), witness(records)) of a statement"""
    if statement == "transfer":
        return (lambda pk, d, r, **kw: circuit.transfer_prove(ctx, pk, DEPTH, d, r, **kw)), lambda d: circuit.transfer_witness(ctx, DEPTH, d)
    if statement == "split":
        return (lambda pk, d, r, **kw: circuit.split_prove(ctx, pk, DEPTH, d, r, **kw)), lambda d: circuit.split_witness(ctx, DEPTH, d)
    return (lambda pk, d, r, **kw: circuit.prove_from_inputs(ctx, pk, DEPTH, d, r, **kw)), lambda d: circuit.witness(ctx, DEPTH, d)


def measure(ctx, statement, args):
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    consts = ctx.mimc7_constants()
    r1 = getattr(circuit, statement + "_r1cs")(consts, DEPTH)
    blob, vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    recs = _records(circuit, statement, args.n, rnd)
    recs_d = ctx.to_device(recs)
    rs = np.frombuffer(b"".join(rnd.randrange(fields.R).to_bytes(32, "little") for _ in range(2 * args.n)), dtype=np.uint8).reshape(args.n, 64).copy()
    prove, witness = _calls(circuit, ctx, statement)
    out = {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d, "n": args.n}
    one_d, one_rs = recs_d[:1].contiguous(), rs[:1]
    out["one_request_ms_min_median_max"] = _mmm(_timed(lambda: prove(pk, one_d, one_rs), args.reps, args.warmup), 3)
    if statement != "withdraw":  # (a): the batch call, transfer beside split
        batch = _timed(lambda: prove(pk, recs_d, rs), args.reps, args.warmup)
        ctx.profile(True)
        proofs, pub = prove(pk, recs_d, rs, return_public=True)
        stages = {k: [round(v[0], 3), v[1]] for k, v in ctx.profile_read().items() if v[1]}
        ctx.profile(False)
        vkb = g16.vk_to_bytes(vk)
        accepted = all(g16.verify(vkb, pub[i], proofs[i].tobytes()) for i in (0, args.n // 2, args.n - 1))
        out.update({"call_ms_min_median_max": _mmm(batch, 2), "proofs_per_s": round(args.n / statistics.median(batch) * 1e3, 1),
                    "sampled_proofs_verify": bool(accepted), "stage_ms_and_launches_of_one_profiled_call": stages})
        del proofs, pub
    pk.close()
    ctx.release_scratch()
    # (c) the witness call alone (it returns after the stream has drained)
    out["witness_ms_min_median_max"] = {"1": _mmm(_timed(lambda: witness(one_d), args.reps, args.warmup), 3),
                                        str(args.n): _mmm(_timed(lambda: witness(recs_d), args.reps, args.warmup), 3)}
    ctx.release_scratch()
    return out, blob, recs[:1], rs[:1]


def lane_local_one_request(api, blob, rec, rs, args):
    """(d) the hooks build with OG_WITNESS_W9=0: one transfer request through k_transfer_core, and the same build's wave-wide walk
    beside it (the hooks library is another binary: its default is measured too, so that the pair is like for like)"""
    from owshen_amd import _lib, circuit, groth16 as g16
    from owshen_amd._abi import bind

    hooks = bind(C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so")))

    class HooksContext(api.Context):
        _lib = hooks

    ctx = HooksContext(0)
    pk = g16.ProvingKey(ctx, blob)
    rec_d = ctx.to_device(rec)
    out = {}
    for name, env in (("wave_wide", None), ("lane_local_OG_WITNESS_W9_0", "0")):
        os.environ.pop("OG_WITNESS_W9", None)
        if env is not None:
            os.environ["OG_WITNESS_W9"] = env
        out[name] = {"one_request_ms_min_median_max": _mmm(_timed(lambda: circuit.transfer_prove(ctx, pk, DEPTH, rec_d, rs), args.reps, args.warmup), 3),
                     "witness_ms_min_median_max": _mmm(_timed(lambda: circuit.transfer_witness(ctx, DEPTH, rec_d), args.reps, args.warmup), 3)}
    os.environ.pop("OG_WITNESS_W9", None)
    pk.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.json"))
    args = ap.parse_args()
    import torch
    from owshen_amd import api
    ctx = api.Context(0)
    out = {"tool": "tools/transfer_bench.py", "depth": DEPTH, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    tele = None
    try:
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.05).start()
    except Exception as e:  # (the numbers stand without it)
        out["telemetry_error"] = repr(e)[:200]
    kept = None
    for statement in STATEMENTS:
        out[statement], blob, rec, rs = measure(ctx, statement, args)
        if statement == "transfer":
            kept = (blob, rec, rs)
        print(statement, json.dumps(out[statement]), flush=True)
    ctx.close()
    out["transfer_hooks_build_one_request"] = lane_local_one_request(api, *kept, args)
    print("hooks", json.dumps(out["transfer_hooks_build_one_request"]), flush=True)
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    w, s, t = out["withdraw"], out["split"], out["transfer"]
    med = lambda d, k: d[k][1]  # noqa: E731
    wit = lambda d, k: d["witness_ms_min_median_max"][k][1]  # noqa: E731
    out["ratios"] = {
        "transfer_over_split_proofs_per_s": round(t["proofs_per_s"] / s["proofs_per_s"], 4),
        "transfer_over_split_wires": round(t["n_wires"] / s["n_wires"], 4),
        "one_request_ms_transfer_over_split": round(med(t, "one_request_ms_min_median_max") / med(s, "one_request_ms_min_median_max"), 4),
        "one_request_ms_transfer_over_withdraw": round(med(t, "one_request_ms_min_median_max") / med(w, "one_request_ms_min_median_max"), 4),
        "witness_ms_transfer_over_withdraw": {k: round(wit(t, k) / wit(w, k), 4) for k in t["witness_ms_min_median_max"]},
        "witness_ms_transfer_over_split": {k: round(wit(t, k) / wit(s, k), 4) for k in t["witness_ms_min_median_max"]},
        "note": "a proofs_per_s ratio below 0.90 is more than twice the added wires; a one-request witness_ms ratio above 1.25 to "
                "withdraw means permutations on the dependent chain that should be beside it: findings to explain",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["ratios"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
