#!/usr/bin/env python3
"""Times og_join_prove_batch_d beside og_split_prove_batch_d and og_withdraw_prove_batch_d on one GPU, in one process, and writes
profiles/join.json.

All three statements at depth 32 (the withdraw statement natural: padding 0 / 0), records device-resident:
 (a) --n requests per call (default 4 096), the median of --reps calls after --warmup calls, and one profiled call's stage times
     (og_profile) for each.  The yardstick is the SPLIT call of the same run: join carries 1.94 x split's wires and hashes on twice
     the domain (2^16), so a ratio (join proofs/s over split proofs/s) below 0.25 is more than twice that extra work and would be a
     finding, to be explained from the stage times;
 (b) the same three statements with ONE request per call;
 (c) og_join_witness_d against og_split_witness_d, for 1 and for --n requests: both chains are 6 + depth gadgets deep (join walks
     its two notes on two lanes), join's even lane also stores the shared wires and runs one inversion, so a ratio above 1.25 at
     one request would mean that the two walks do not run side by side.
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/join_bench.py [--n 4096] [--reps 5] [--warmup 2] [--out profiles/join.json]"""
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


def _join_records(ctx, n, rng):
    """n well-formed join records whose two notes meet at level 0: each note's first sibling is the other's leaf (computed with
    og_mimc7_hash2_d), the 31 siblings above are shared"""
    recs = rng.integers(0, 256, (n, 11 + 2 * DEPTH, 32), dtype=np.uint8)
    recs[:, :, 31] &= 0x1F                       # every field < 2^253 < r
    recs[:, (2, 6), 8:] = 0                      # amounts < 2^64
    recs[:, (3, 7), 4:] = 0                      # indices < 2^32
    recs[:, 3, 0] &= 0xFE
    recs[:, 7] = recs[:, 3]
    recs[:, 7, 0] |= 0x01
    recs[:, 11 + DEPTH + 1:] = recs[:, 11 + 1:11 + DEPTH]

    def h2(l, r):
        return ctx.to_host(ctx.mimc7_hash2(ctx.to_device(np.ascontiguousarray(l)), ctx.to_device(np.ascontiguousarray(r))))

    leaf = [h2(h2(recs[:, o], recs[:, o + 1]), h2(recs[:, o + 2], recs[:, 8])) for o in (0, 4)]
    recs[:, 11] = leaf[1]
    recs[:, 11 + DEPTH] = leaf[0]
    return recs


def _records(ctx, circuit, statement, n, rnd, rng):
    from oracle.py import fields
    if statement == "join":
        return _join_records(ctx, n, rng)
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


def _mmm(times, digits):
    return [round(min(times), digits), round(statistics.median(times), digits), round(max(times), digits)]


def measure(ctx, statement, args):
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    rng = np.random.default_rng(4096)
    consts = ctx.mimc7_constants()
    r1 = {"join": lambda: circuit.join_r1cs(consts, DEPTH), "split": lambda: circuit.split_r1cs(consts, DEPTH),
          "withdraw": lambda: circuit.withdraw_r1cs(consts, DEPTH, 0, 0)}[statement]()
    blob, vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    recs_d = ctx.to_device(_records(ctx, circuit, statement, args.n, rnd, rng))
    rs = np.frombuffer(b"".join(rnd.randrange(fields.R).to_bytes(32, "little") for _ in range(2 * args.n)), dtype=np.uint8).reshape(args.n, 64).copy()

    def prove(d, r, **kw):
        if statement == "join":
            return circuit.join_prove(ctx, pk, DEPTH, d, r, **kw)
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
    out = {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d, "n": args.n,
           "call_ms_min_median_max": _mmm(batch, 2), "proofs_per_s": round(args.n / statistics.median(batch) * 1e3, 1),
           "one_request_ms_min_median_max": _mmm(one, 3), "sampled_proofs_verify": bool(accepted),
           "stage_ms_and_launches_of_one_profiled_call": stages}
    if statement in ("join", "split"):  # (c) the witness call alone (it returns after the stream has drained)
        witness = circuit.join_witness if statement == "join" else circuit.split_witness
        del proofs, pub
        pk.close()
        pk = None
        ctx.release_scratch()
        out["witness_ms_min_median_max"] = {"1": _mmm(_timed(lambda: witness(ctx, DEPTH, one_d), args.reps, args.warmup), 3),
                                            str(args.n): _mmm(_timed(lambda: witness(ctx, DEPTH, recs_d), args.reps, args.warmup), 3)}
    if pk is not None:
        pk.close()
    ctx.release_scratch()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join.json"))
    args = ap.parse_args()
    import torch
    from owshen_amd import api
    ctx = api.Context(0)
    out = {"tool": "tools/join_bench.py", "depth": DEPTH, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for statement in ("withdraw", "split", "join"):
        out[statement] = measure(ctx, statement, args)
        print(statement, json.dumps(out[statement]), flush=True)
    ctx.close()
    s, j = out["split"], out["join"]
    wj, ws = j["witness_ms_min_median_max"], s["witness_ms_min_median_max"]
    out["join_over_split"] = {"proofs_per_s": round(j["proofs_per_s"] / s["proofs_per_s"], 4),
                              "one_request_ms": round(j["one_request_ms_min_median_max"][1] / s["one_request_ms_min_median_max"][1], 4),
                              "wires": round(j["n_wires"] / s["n_wires"], 4),
                              "witness_ms": {k: round(wj[k][1] / ws[k][1], 4) for k in wj},
                              "note": "a proofs_per_s ratio below 0.25 is more than twice the extra work of the statement; a witness_ms "
                                      "ratio above 1.25 at one request means the two walks do not run side by side: findings to explain"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["join_over_split"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
