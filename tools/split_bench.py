#!/usr/bin/env python3
"""Times og_split_prove_batch_d beside og_withdraw_prove_batch_d on one GPU, in one process, and writes profiles/split.json.

Both statements at depth 32 (the withdraw statement natural: padding 0 / 0), records device-resident: --n requests per call
(default 4 096), the median of --reps calls after --warmup calls, and the same for ONE request per call.  The yardstick is the
withdraw call of the same run: split carries +6.5 % wires and +5.6 % hashes on the same 2^15 domain, so a ratio (split proofs/s over
withdraw proofs/s) below 0.85 is more than twice that extra work and would be a finding; the stage times of one profiled call of
each statement (og_profile) are recorded beside the rates to explain it.  Recorded, not gated: the script always exits 0 after a
complete run.

    python tools/split_bench.py [--n 4096] [--reps 5] [--warmup 2] [--out profiles/split.json]"""
import argparse
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


def _records(circuit, statement, n, rnd):
    from oracle.py import fields
    recs = []
    for _ in range(n):
        amount = rnd.randrange(1, 1 << 64)
        common = dict(nullifier=rnd.randrange(fields.R), secret=rnd.randrange(fields.R), amount=amount, recipient=rnd.randrange(1 << 160),
                      index=rnd.randrange(1 << DEPTH), siblings=[rnd.randrange(fields.R) for _ in range(DEPTH)],
                      token=rnd.randrange(1 << 160), chain_id=rnd.randrange(1 << 32))
        if statement == "split":
            recs.append(circuit.pack_split_inputs(amount_out=rnd.randrange(amount + 1), change_commitment=rnd.randrange(fields.R), **common))
        else:
            recs.append(circuit.pack_inputs(pad_seed=0, **common))
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


def measure(ctx, statement, args):
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    consts = ctx.mimc7_constants()
    r1 = circuit.split_r1cs(consts, DEPTH) if statement == "split" else circuit.withdraw_r1cs(consts, DEPTH, 0, 0)
    blob, vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    recs_d = ctx.to_device(_records(circuit, statement, args.n, rnd))
    rs = np.frombuffer(b"".join(rnd.randrange(fields.R).to_bytes(32, "little") for _ in range(2 * args.n)), dtype=np.uint8).reshape(args.n, 64).copy()

    def prove(d, r, **kw):
        if statement == "split":
            return circuit.split_prove(ctx, pk, DEPTH, d, r, **kw)
        return circuit.prove_from_inputs(ctx, pk, DEPTH, d, r, **kw)

    batch = _timed(lambda: prove(recs_d, rs), args.reps, args.warmup)
    one_d, one_rs = recs_d[:1].contiguous(), rs[:1]
    one = _timed(lambda: prove(one_d, one_rs), args.reps, args.warmup)
    ctx.profile(True)
    proofs, pub = prove(recs_d, rs, return_public=True)
    stages = {k: [round(v[0], 3), v[1]] for k, v in ctx.profile_read().items() if v[1]}
    ctx.profile(False)
    vkb = g16.vk_to_bytes(vk)
    accepted = all(g16.verify(vkb, pub[i], proofs[i].tobytes()) for i in (0, args.n // 2, args.n - 1))
    pk.close()
    ctx.release_scratch()
    med = statistics.median(batch)
    return {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d, "n": args.n,
            "call_ms_min_median_max": [round(min(batch), 2), round(med, 2), round(max(batch), 2)],
            "proofs_per_s": round(args.n / med * 1e3, 1),
            "one_request_ms_min_median_max": [round(min(one), 3), round(statistics.median(one), 3), round(max(one), 3)],
            "sampled_proofs_verify": bool(accepted), "stage_ms_and_launches_of_one_profiled_call": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split.json"))
    args = ap.parse_args()
    from owshen_amd import api
    ctx = api.Context(0)
    out = {"tool": "tools/split_bench.py", "depth": DEPTH, "reps": args.reps, "warmup": args.warmup, "measured_on_gpu": True}
    for statement in ("withdraw", "split"):
        out[statement] = measure(ctx, statement, args)
        print(statement, json.dumps(out[statement]), flush=True)
    ctx.close()
    w, s = out["withdraw"], out["split"]
    out["split_over_withdraw"] = {"proofs_per_s": round(s["proofs_per_s"] / w["proofs_per_s"], 4),
                                  "one_request_ms": round(s["one_request_ms_min_median_max"][1] / w["one_request_ms_min_median_max"][1], 4),
                                  "wires": round(s["n_wires"] / w["n_wires"], 4),
                                  "note": "a proofs_per_s ratio below 0.85 is more than twice the extra work of the statement: a finding to explain"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["split_over_withdraw"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
