#!/usr/bin/env python3
"""Times the view-key calls beside their nearest neighbours, on one GPU, in one process, and writes profiles/view_notes.json.

The median of --reps calls after --warmup warm calls, the two sides of a pair taking turns inside every repetition; engine clock and
socket power sampled on the host while the run lasts (bench.py GpuTelemetry).  The yardstick is always the neighbour in the SAME run:
 (a) og_note_scan_view_batch_d beside og_note_scan_owned_batch_d at 65 536 and 2^20 memos: the same seal requests sealed in either
     form (one memo in 1 024 the scanner's, leaves beside the memos), scanned by the key that owns those and by a key that owns none;
     and, since a memo nobody owns is the same work whatever its form, both scans with the stranger's key over the VIEW memos -- the
     same bytes.  The hit-free view scan executes the owned scan's front with another tag index, so that ratio should lie within the
     spread of the owned scan's own repetitions (recorded beside it as max / min);
 (b) og_note_unlock_batch_d beside og_eddsa_pubkey_batch_d at 65 536 rows: both are 64 table additions and an inversion; unlock adds
     two permutations for c and, with leaves, four for the leaf;
 (c) og_note_seal_view_batch_d beside og_note_seal_owned_batch_d at 65 536 requests.
Recorded, not gated: the script always exits 0 after a complete run.

    python tools/view_notes_bench.py [--sizes 65536,1048576] [--rows 65536] [--reps 10] [--warmup 1] [--out profiles/view_notes.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

ONE_IN = 1024


def _pairs(calls, reps, warmup):
    """calls: name -> callable; every repetition runs each once, in turn -> name -> [min, median, max] ms"""
    for _ in range(warmup):
        for call in calls.values():
            call()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: [round(min(t), 3), round(statistics.median(t), 3), round(max(t), 3)] for name, t in times.items()}


def _ratio(pair, a, b):
    return round(pair[a][1] / pair[b][1], 4)


def _spread(mmm):
    return round(mmm[2] / mmm[0], 4)


def measure_scans(ctx, n, args):
    from note_scan_bench import _keys, seal_requests
    sks, pks = _keys(ctx, 1)      # sks: the scanner (view scalar and owned sk alike), the owner of every other memo, a stranger
    spend, spend_pk = _keys(ctx, 2)   # the scanner's spend scalar first; its key is the second point of every view request
    ps = bytes(spend_pk[0])
    req5 = seal_requests(pks, n, 4)
    req7 = np.zeros((n, 7, 32), dtype=np.uint8)
    req7[:, :3], req7[:, 3:5], req7[:, 5:] = req5[:, :3], spend_pk[0].reshape(2, 32), req5[:, 3:]
    want = np.zeros(n, dtype=np.uint32)
    want[::ONE_IN] = 1
    o_memos, o_notes, ok = ctx.note_seal_owned(ctx.to_device(req5))
    assert ok.all(), "a seeded owned seal request was refused"
    v_memos, v_notes, ok = ctx.note_seal_view(ctx.to_device(req7))
    assert ok.all(), "a seeded view seal request was refused"
    o_leaves, v_leaves = o_notes[:, 1, :].contiguous(), v_notes[:, 1, :].contiguous()
    del o_notes, v_notes
    owned = lambda key, memos, leaves: ctx.note_scan_owned(key, memos, leaves)  # noqa: E731
    view = lambda key, memos, leaves: ctx.note_scan_view(key, ps, memos, leaves)  # noqa: E731
    assert np.array_equal(owned(sks[0], o_memos, o_leaves)[1], want) and np.array_equal(view(sks[0], v_memos, v_leaves)[1], want)
    for scan in (owned, view):
        for memos, leaves in ((o_memos, o_leaves), (v_memos, v_leaves)):
            assert not scan(sks[2], memos, leaves)[1].any()
    # what a service hands back, and the wallet unlocks: every hit, none else
    rows, _hit = view(sks[0], v_memos, v_leaves)
    unlocked, ok = ctx.note_unlock(spend[0], rows, v_leaves)
    assert np.array_equal(ok, want), "a hit of the scan did not unlock"
    del rows, unlocked
    out = {"n": n, "hits": int(want.sum())}
    out["one_hit_in_1024_ms_min_median_max"] = _pairs({"scan_owned": lambda: owned(sks[0], o_memos, o_leaves),
                                                       "scan_view": lambda: view(sks[0], v_memos, v_leaves)}, args.reps, args.warmup)
    out["no_hits_ms_min_median_max"] = _pairs({"scan_owned": lambda: owned(sks[2], o_memos, o_leaves),
                                               "scan_view": lambda: view(sks[2], v_memos, v_leaves)}, args.reps, args.warmup)
    out["no_hits_same_memos_ms_min_median_max"] = _pairs({"scan_owned": lambda: owned(sks[2], v_memos, v_leaves),
                                                          "scan_view": lambda: view(sks[2], v_memos, v_leaves)}, args.reps, args.warmup)
    out["memos_per_s_scan_view_one_hit_in_1024"] = round(n / out["one_hit_in_1024_ms_min_median_max"]["scan_view"][1] * 1e3)
    out["ratios_view_over_owned"] = {k.replace("_ms_min_median_max", ""): _ratio(out[k], "scan_view", "scan_owned")
                                     for k in list(out) if k.endswith("_ms_min_median_max")}
    out["owned_scan_own_spread_max_over_min"] = {k.replace("_ms_min_median_max", ""): _spread(out[k]["scan_owned"])
                                                 for k in list(out) if k.endswith("_ms_min_median_max")}
    return out


def measure_unlock_and_seal(ctx, args):
    from note_scan_bench import _keys, seal_requests
    n = args.rows
    sks, pks = _keys(ctx, 1)
    spend, spend_pk = _keys(ctx, 2)
    ps = bytes(spend_pk[0])
    req5 = seal_requests(np.stack([pks[0], pks[0]]), n, 5)   # every memo the scanner's: every row unlocks
    req7 = np.zeros((n, 7, 32), dtype=np.uint8)
    req7[:, :3], req7[:, 3:5], req7[:, 5:] = req5[:, :3], spend_pk[0].reshape(2, 32), req5[:, 3:]
    req5_d, req7_d = ctx.to_device(req5), ctx.to_device(req7)
    memos, notes, ok = ctx.note_seal_view(req7_d)
    assert ok.all()
    leaves = notes[:, 1, :].contiguous()
    rows, hit = ctx.note_scan_view(sks[0], ps, memos, leaves)
    assert (hit == 1).all()
    assert ctx.note_unlock(spend[0], rows, leaves)[1].all() and ctx.note_unlock(spend[0], rows, None)[1].all()
    scalars = ctx.to_device(np.ascontiguousarray(req5[:, 0]))   # n canonical scalars for the key derivation
    out = {"n": n}
    out["unlock_ms_min_median_max"] = _pairs({"eddsa_pubkey": lambda: ctx.eddsa_pubkey(scalars, compressed=False),
                                              "unlock": lambda: ctx.note_unlock(spend[0], rows, None),
                                              "unlock_with_leaves": lambda: ctx.note_unlock(spend[0], rows, leaves)}, args.reps, args.warmup)
    out["seal_ms_min_median_max"] = _pairs({"seal_owned": lambda: ctx.note_seal_owned(req5_d),
                                            "seal_view": lambda: ctx.note_seal_view(req7_d)}, args.reps, args.warmup)
    out["ratios"] = {"unlock_over_eddsa_pubkey": _ratio(out["unlock_ms_min_median_max"], "unlock", "eddsa_pubkey"),
                     "unlock_with_leaves_over_eddsa_pubkey": _ratio(out["unlock_ms_min_median_max"], "unlock_with_leaves", "eddsa_pubkey"),
                     "seal_view_over_seal_owned": _ratio(out["seal_ms_min_median_max"], "seal_view", "seal_owned")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_notes.json"))
    args = ap.parse_args()
    import torch
    from owshen_amd import api

    ctx = api.Context(0)
    out = {"tool": "tools/view_notes_bench.py", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "yardstick": "og_note_scan_owned_batch_d / og_eddsa_pubkey_batch_d / og_note_seal_owned_batch_d in the same run, taking turns"}
    tele = None
    try:
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.05).start()
    except Exception as e:  # (the numbers stand without it)
        out["telemetry_error"] = repr(e)[:200]
    out["scans"] = {}
    for n in (int(s) for s in args.sizes.split(",")):
        out["scans"][str(n)] = measure_scans(ctx, n, args)
        print("scans", n, json.dumps(out["scans"][str(n)]), flush=True)
        ctx.release_scratch()
    out["unlock_and_seal"] = measure_unlock_and_seal(ctx, args)
    print("unlock_and_seal", json.dumps(out["unlock_and_seal"]), flush=True)
    ctx.close()
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
