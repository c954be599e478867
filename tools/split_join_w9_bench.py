#!/usr/bin/env python3
"""Times the wave-wide witness walk of the split and the join statement (k_sw9_*, k_jw9_*) beside withdraw's and transfer's on one GPU,
in one process, and writes profiles/split_join_w9.json.  profiles/split.json, join.json and transfer.json stay the record they are.

All four statements at depth 32 (the withdraw statement natural: padding 0 / 0), records device-resident, the median of --reps calls
after --warmup calls; engine clock and socket power sampled on the host while the run lasts (bench.py GpuTelemetry).  Every yardstick
but (d)'s is another call of the SAME run:
 (a) ONE request per call through the *_prove_batch_d calls, for withdraw, transfer, split and join;
 (b) the witness call alone, for 1 request and for --w9-n requests (default 512: the largest call that takes the wave-wide walk);
 (c) the lane-local yardstick: one request of split and of join through the hooks build with OG_WITNESS_W9=0 (k_split_core,
     k_join_core), and the same build's wave-wide walk beside it (the hooks library is another binary: the pair is like for like);
 (d) the batch check: --n requests per call (default 4 096) of split and of join, which do NOT take the new path, against
     profiles/split.json and profiles/join.json as the parent commit left them, scaled by the box index of the run -- the withdraw
     call of --n requests of this run over the one those files recorded beside their own numbers (no code of that call changed).
Ratios: for one request, the witness call of split and of join over og_withdraw_witness_d and over og_transfer_witness_d.  The
dependent chain of all four is the same 4 + depth + #left permutations, so above 1.25 to withdraw is a finding to be explained from
the launches: split's margin covers the wider first two launches and 6.5 % more wires to convert; join converts 2.07 x withdraw's
wires and its first launch is twice as wide, so its excess, if any, belongs to k_wires_from_limbs and to the launches' width, not to
the chain (tools/split_join_w9_trace.py under `rocprofv3 --kernel-trace --stats` shows each kernel's share: a run of its own).
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/split_join_w9_bench.py [--n 4096] [--w9-n 512] [--reps 5] [--warmup 1] [--out profiles/split_join_w9.json]"""
import argparse
import ctypes as C
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.join_bench import _join_records  # noqa: E402
from tools.transfer_bench import _mmm, _records, _timed  # noqa: E402

DEPTH = 32
STATEMENTS = ("withdraw", "transfer", "split", "join")
BATCHED = ("withdraw", "split", "join")   # withdraw: the box index


def _calls(circuit, ctx, statement):
    """(prove(pk, records, rs), witness(records)) of a statement"""
    if statement == "withdraw":
        return (lambda pk, d, r: circuit.prove_from_inputs(ctx, pk, DEPTH, d, r)), lambda d: circuit.witness(ctx, DEPTH, d)
    prove, witness = getattr(circuit, statement + "_prove"), getattr(circuit, statement + "_witness")
    return (lambda pk, d, r: prove(ctx, pk, DEPTH, d, r)), lambda d: witness(ctx, DEPTH, d)


def measure(ctx, statement, args):
    from oracle.py import fields
    from owshen_amd import circuit, groth16 as g16
    rnd = random.Random(4096)
    r1 = getattr(circuit, statement + "_r1cs")(ctx.mimc7_constants(), DEPTH)
    blob, _vk = g16.setup(ctx, r1, 5, 6, 7, 8, 9)
    pk = g16.ProvingKey(ctx, blob)
    n = args.n if statement in BATCHED else args.w9_n
    recs = _join_records(ctx, n, np.random.default_rng(4096)) if statement == "join" else _records(circuit, statement, n, rnd)
    recs_d = ctx.to_device(recs)
    rs = np.frombuffer(b"".join(rnd.randrange(fields.R).to_bytes(32, "little") for _ in range(2 * n)), dtype=np.uint8).reshape(n, 64).copy()
    prove, witness = _calls(circuit, ctx, statement)
    out = {"n_wires": r1.n_wires, "n_constraints": r1.n_constraints, "n_pub": r1.n_pub, "log_d": r1.log_d}
    one_d, one_rs = recs_d[:1].contiguous(), rs[:1]
    out["one_request_ms_min_median_max"] = _mmm(_timed(lambda: prove(pk, one_d, one_rs), args.reps, args.warmup), 3)   # (a)
    if statement in BATCHED:                                                                                           # (d)
        batch = _timed(lambda: prove(pk, recs_d, rs), args.reps, args.warmup)
        out.update({"n": n, "call_ms_min_median_max": _mmm(batch, 2), "proofs_per_s": round(n / _mmm(batch, 6)[1] * 1e3, 1)})
    pk.close()
    ctx.release_scratch()
    many_d = recs_d[:args.w9_n].contiguous()                                                                           # (b)
    out["witness_ms_min_median_max"] = {"1": _mmm(_timed(lambda: witness(one_d), args.reps, args.warmup), 3),
                                        str(args.w9_n): _mmm(_timed(lambda: witness(many_d), args.reps, args.warmup), 3)}
    ctx.release_scratch()
    return out, blob, recs[:1], rs[:1]


def hooks_build_one_request(api, kept, args):
    """(c) one request of split and of join through the hooks build: its default (the wave-wide walk) and OG_WITNESS_W9=0"""
    from owshen_amd import _lib, circuit, groth16 as g16
    from owshen_amd._abi import bind

    hooks = bind(C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so")))

    class HooksContext(api.Context):
        _lib = hooks

    ctx = HooksContext(0)
    out = {}
    for statement, (blob, rec, rs) in kept.items():
        pk = g16.ProvingKey(ctx, blob)
        rec_d = ctx.to_device(rec)
        prove, witness = _calls(circuit, ctx, statement)
        out[statement] = {}
        for name, env in (("wave_wide", None), ("lane_local_OG_WITNESS_W9_0", "0")):
            os.environ.pop("OG_WITNESS_W9", None)
            if env is not None:
                os.environ["OG_WITNESS_W9"] = env
            out[statement][name] = {"one_request_ms_min_median_max": _mmm(_timed(lambda: prove(pk, rec_d, rs), args.reps, args.warmup), 3),
                                    "witness_ms_min_median_max": _mmm(_timed(lambda: witness(rec_d), args.reps, args.warmup), 3)}
        os.environ.pop("OG_WITNESS_W9", None)
        pk.close()
        ctx.release_scratch()
    ctx.close()
    return out


def batch_check(out):
    """(d) this run's batch calls of split and join against the recorded ones, scaled by the box index"""
    check = {}
    for statement in ("split", "join"):
        path = os.path.join(ROOT, "profiles", statement + ".json")
        try:
            with open(path) as f:
                then = json.load(f)
            if then[statement]["n"] != out[statement]["n"]:
                raise ValueError(f"recorded for {then[statement]['n']} requests per call")
            box = out["withdraw"]["call_ms_min_median_max"][1] / then["withdraw"]["call_ms_min_median_max"][1]
            was, now = then[statement]["call_ms_min_median_max"][1], out[statement]["call_ms_min_median_max"][1]
            check[statement] = {"recorded_call_ms": was, "box_index_withdraw_call_now_over_recorded": round(box, 4),
                                "recorded_call_ms_scaled": round(was * box, 2), "call_ms": now, "call_ms_over_scaled": round(now / (was * box), 4)}
        except (OSError, KeyError, ValueError) as e:
            check[statement] = {"error": repr(e)[:200]}
    return check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--w9-n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_join_w9.json"))
    args = ap.parse_args()
    assert args.w9_n <= args.n
    import torch
    from owshen_amd import api
    ctx = api.Context(0)
    out = {"tool": "tools/split_join_w9_bench.py", "depth": DEPTH, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    tele = None
    try:
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.05).start()
    except Exception as e:  # (the numbers stand without it)
        out["telemetry_error"] = repr(e)[:200]
    kept = {}
    for statement in STATEMENTS:
        out[statement], blob, rec, rs = measure(ctx, statement, args)
        if statement in ("split", "join"):
            kept[statement] = (blob, rec, rs)
        print(statement, json.dumps(out[statement]), flush=True)
    ctx.close()
    out["hooks_build_one_request"] = hooks_build_one_request(api, kept, args)
    print("hooks", json.dumps(out["hooks_build_one_request"]), flush=True)
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    out["batch_check"] = batch_check(out)
    wit = lambda s, k: out[s]["witness_ms_min_median_max"][k][1]  # noqa: E731
    one = lambda s: out[s]["one_request_ms_min_median_max"][1]  # noqa: E731
    hooks = out["hooks_build_one_request"]
    ratios = {}
    for s in ("split", "join"):
        ratios[s] = {
            "witness_ms_one_request_over_withdraw": round(wit(s, "1") / wit("withdraw", "1"), 4),
            "witness_ms_one_request_over_transfer": round(wit(s, "1") / wit("transfer", "1"), 4),
            f"witness_ms_{args.w9_n}_requests_over_withdraw": round(wit(s, str(args.w9_n)) / wit("withdraw", str(args.w9_n)), 4),
            f"witness_ms_{args.w9_n}_requests_over_transfer": round(wit(s, str(args.w9_n)) / wit("transfer", str(args.w9_n)), 4),
            "one_request_ms_over_withdraw": round(one(s) / one("withdraw"), 4),
            "one_request_ms_over_transfer": round(one(s) / one("transfer"), 4),
            "wires_over_withdraw": round(out[s]["n_wires"] / out["withdraw"]["n_wires"], 4),
            "wires_over_transfer": round(out[s]["n_wires"] / out["transfer"]["n_wires"], 4),
            "hooks_build_wave_wide_over_lane_local_witness_ms": round(
                hooks[s]["wave_wide"]["witness_ms_min_median_max"][1] / hooks[s]["lane_local_OG_WITNESS_W9_0"]["witness_ms_min_median_max"][1], 4),
            "hooks_build_wave_wide_over_lane_local_one_request_ms": round(
                hooks[s]["wave_wide"]["one_request_ms_min_median_max"][1] / hooks[s]["lane_local_OG_WITNESS_W9_0"]["one_request_ms_min_median_max"][1], 4),
        }
    ratios["note"] = ("a one-request witness_ms ratio above 1.25 to withdraw means permutations on the dependent chain that should be beside "
                      "it, or a conversion / launch width that shows: a finding to explain from the launches")
    out["ratios"] = ratios
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["ratios"]))
    print(json.dumps(out["batch_check"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
