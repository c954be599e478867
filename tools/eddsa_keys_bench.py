#!/usr/bin/env python3
"""Times the four BabyJubJub key calls against og_eddsa_verify_batch_d on one box, in one process, and writes
profiles/eddsa_keys.json.

For n in {4096, 65536}: n seeded sign requests are signed on the device; the records that come back are the batch every call is
timed on, device-resident -- og_eddsa_verify_batch_d on them (the yardstick: unchanged by the calls under test), then
og_eddsa_verify_compressed_batch_d on the same records with their keys compressed, og_eddsa_sign_batch_d on the requests,
og_eddsa_decompress_batch_d on the compressed keys and og_eddsa_pubkey_batch_d on the secret keys.  One warm call of each, then
--reps rounds that time the five calls in turn (so that a drifting clock touches them alike); a time is a host clock around a call
that ends in the copy of its decisions, i.e. in a stream synchronise.  Reported: min / median / max per call, the ratio of the
medians to the yardstick's, and the engine clock and socket power sampled on the host while the run lasts (bench.py
GpuTelemetry).  Findings (ISSUE "Measurement"): verify_compressed / verify > 1.5, or sign slower than verify; recorded, not gated.

    python tools/eddsa_keys_bench.py [--sizes 4096,65536] [--reps 5] [--out profiles/eddsa_keys.json]"""
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

CALLS = ("verify", "verify_compressed", "sign", "decompress", "pubkey")


def _requests(n, seed):
    from owshen_amd.api import FR_MODULUS as R
    rnd = random.Random(seed)
    raw = b"".join(rnd.randrange(1, R).to_bytes(32, "little") for _ in range(3 * n))
    return np.frombuffer(raw, dtype=np.uint8).reshape(n, 3, 32).copy()


def _compressed(recs):
    """[n, 6, 32] records -> [n, 5, 32]: the parity of pk.y into bit 255 of pk.x"""
    out = np.ascontiguousarray(recs[:, 1:, :]).copy()
    out[:, 0, :] = recs[:, 0, :]
    out[:, 0, 31] |= (recs[:, 1, 0] & 1) << 7
    return out


def measure(ctx, n, reps, seed=1):
    reqs = _requests(n, seed)
    reqs_d = ctx.to_device(reqs)
    recs_d, ok = ctx.eddsa_sign(reqs_d)
    assert ok.all(), "a seeded request was refused"
    recs = np.asarray(ctx.to_host(recs_d)).reshape(n, 6, 32)
    crecs_d = ctx.to_device(_compressed(recs))
    pkc_d = ctx.to_device(np.ascontiguousarray(_compressed(recs)[:, 0, :]))
    sks_d = ctx.to_device(np.ascontiguousarray(reqs[:, 0, :]))
    run = {"verify": lambda: ctx.eddsa_verify(recs_d), "verify_compressed": lambda: ctx.eddsa_verify_compressed(crecs_d),
           "sign": lambda: ctx.eddsa_sign(reqs_d)[1], "decompress": lambda: ctx.eddsa_decompress(pkc_d)[1],
           "pubkey": lambda: ctx.eddsa_pubkey(sks_d)[2]}
    for name in CALLS:   # warm, and every decision of an honest batch is an accept
        assert run[name]().all(), name
    pk, _ = ctx.eddsa_decompress(pkc_d)
    assert np.array_equal(np.asarray(ctx.to_host(pk)).reshape(n, 2, 32), recs[:, :2, :]), "decompress(compress(pk)) != pk"
    times = {name: [] for name in CALLS}
    for _ in range(reps):
        for name in CALLS:
            t0 = time.perf_counter()
            run[name]()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(times[name]) for name in CALLS}
    row = {"n": n, "ms_min_median_max": {name: [round(min(t), 3), round(med[name], 3), round(max(t), 3)] for name, t in times.items()},
           "per_s": {name: round(n / med[name] * 1e3) for name in CALLS},
           "ratio_to_verify": {name: round(med[name] / med["verify"], 3) for name in CALLS if name != "verify"}}
    row["findings"] = [f for f, hit in (("verify_compressed / verify > 1.5", row["ratio_to_verify"]["verify_compressed"] > 1.5),
                                        ("sign slower than verify", row["ratio_to_verify"]["sign"] > 1.0)) if hit]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eddsa_keys.json"))
    args = ap.parse_args()
    from owshen_amd import api
    ctx = api.Context(0)
    out = {"tool": "tools/eddsa_keys_bench.py", "reps": args.reps, "warm_calls": 1, "measured_on_gpu": True,
           "yardstick": "og_eddsa_verify_batch_d on the same records in the same run", "sizes": []}
    tele = None
    try:
        import torch
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.02).start()
    except Exception as e:   # the helper is optional
        out["telemetry_error"] = repr(e)[:200]
    for n in (int(s) for s in args.sizes.split(",")):
        row = measure(ctx, n, args.reps)
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
