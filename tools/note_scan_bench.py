#!/usr/bin/env python3
"""Times og_note_scan_batch_d and og_note_seal_batch_d against og_eddsa_verify_batch_d on one box, in one process, and writes
profiles/note_scan.json.

Scan: n memos sealed on the device (og_note_seal_batch_d) with one memo in 1 024 sealed to the scanning key and the rest to another
key; memos, published leaves and the opened rows are device-resident, the call ends in the copy of its n hit codes.  The same memos are
also scanned with a key that owns none of them (scan_no_hits): a wave that holds a hit runs fourteen permutations where the others run
four, and at one wave per SIMD a call lasts as long as its slowest wave.  Sizes 65 536 and
2^20 (the tree of BASELINE.json configs[4]).  Seal: 65 536 requests.  The yardstick, in the same run: og_eddsa_verify_batch_d on 65 536
signed records (the existing kernel closest in kind), and on 2^20 so that the large scan has a like-for-like partner.  One warm call
of each, then --reps rounds that time the calls in turn (a drifting clock touches them alike); a time is a host clock around a call
that ends in a stream synchronise.  Reported: min / median / max ms per call, items per second, the per-item ratio scan / verify, and
the engine clock and socket power sampled on the host while the run lasts (bench.py GpuTelemetry).

A/B (the hooks build, same memos, same process): the shipped form (width-4 NAF, a table of four, the dedicated doubling) against the
same call with the doubling replaced by the unified law (OG_NOTE_DBL_UNIFIED=1) and against the width-3 NAF with a table of two
(OG_NOTE_NAF_W=3: fewer registers, one more wave per SIMD, thirteen more additions).

    python tools/note_scan_bench.py [--sizes 65536,1048576] [--reps 10] [--out profiles/note_scan.json]"""
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

ONE_IN = 1024
AB_FORMS = (("shipped", {}), ("unified_doubling", {"OG_NOTE_DBL_UNIFIED": "1"}), ("naf3_table_of_two", {"OG_NOTE_NAF_W": "3"}))
AB_ENV = ("OG_NOTE_DBL_UNIFIED", "OG_NOTE_NAF_W")


def _field_bytes(rng, n):
    """n x 32 random bytes below 2^253 (every one a canonical field element)"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x1F
    return a


def _keys(ctx, seed):
    from owshen_amd.api import FR_MODULUS as R
    rnd = random.Random(seed)
    sks = [rnd.randrange(1, R) for _ in range(3)]   # the scanner, the owner of every other memo, a stranger who owns none
    raw = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in sks[:2]), dtype=np.uint8).reshape(2, 32).copy()
    pk, _c, ok = ctx.eddsa_pubkey(ctx.to_device(raw), compressed=False)
    assert ok.all()
    return sks, np.asarray(ctx.to_host(pk)).reshape(2, 64)


def seal_requests(pks, n, seed):
    rng = np.random.default_rng(seed)
    req = np.zeros((n, 5, 32), dtype=np.uint8)
    req[:, 0] = _field_bytes(rng, n)
    req[:, 0, 0] |= 1                                   # e != 0
    req[:, 1:3] = pks[1].reshape(2, 32)
    req[::ONE_IN, 1:3] = pks[0].reshape(2, 32)
    req[:, 3, :8] = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    req[:, 4, :20] = rng.integers(0, 256, size=(n, 20), dtype=np.uint8)
    return req


def verify_records(ctx, n, seed):
    rng = np.random.default_rng(seed)
    reqs = np.stack([_field_bytes(rng, n) for _ in range(3)], axis=1)
    recs_d, ok = ctx.eddsa_sign(ctx.to_device(reqs))
    assert ok.all(), "a seeded sign request was refused"
    return recs_d


def _timed(run, names, reps):
    times = {name: [] for name in names}
    for _ in range(reps):
        for name in names:
            t0 = time.perf_counter()
            run[name]()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def _row(times, items):
    med = {k: statistics.median(t) for k, t in times.items()}
    return {"ms_min_median_max": {k: [round(min(t), 3), round(med[k], 3), round(max(t), 3)] for k, t in times.items()},
            "per_s": {k: round(items[k] / med[k] * 1e3) for k in times}}, med


def measure(ctx, hctx, sizes, reps, seed=1):
    sks, pks = _keys(ctx, seed)
    n_seal = n_verify = 65536
    out = {"sizes": []}
    seal_d = ctx.to_device(seal_requests(pks, n_seal, seed + 1))
    recs_d = verify_records(ctx, n_verify, seed + 2)
    assert ctx.eddsa_verify(recs_d).all()
    for n in sizes:
        memos_d, notes_d, ok = ctx.note_seal(ctx.to_device(seal_requests(pks, n, seed + 3)))
        assert ok.all(), "a seeded seal request was refused"
        leaves_d = notes_d[:, 1, :].contiguous()
        want = np.zeros(n, dtype=np.uint32)
        want[::ONE_IN] = 1
        big_d = recs_d if n == n_verify else verify_records(ctx, n, seed + 4)
        run = {"scan": lambda: ctx.note_scan(sks[0], memos_d, leaves_d)[1], "scan_no_hits": lambda: ctx.note_scan(sks[2], memos_d, leaves_d)[1],
               "verify": lambda: ctx.eddsa_verify(big_d),
               "verify_65536": lambda: ctx.eddsa_verify(recs_d), "seal_65536": lambda: ctx.note_seal(seal_d)[2]}
        assert np.array_equal(run["scan"](), want), "the scan's hits are not the one memo in %d sealed to the key" % ONE_IN
        assert not run["scan_no_hits"]().any()
        assert run["verify"]().all() and run["verify_65536"]().all() and run["seal_65536"]().all()   # (the warm calls)
        opened_d, _h = ctx.note_scan(sks[0], memos_d, leaves_d)
        opened = np.asarray(ctx.to_host(opened_d)).reshape(n, 4, 32)
        assert opened[::ONE_IN].any(axis=(1, 2)).all() and not np.delete(opened, np.s_[::ONE_IN], axis=0).any()
        items = {"scan": n, "scan_no_hits": n, "verify": n, "verify_65536": n_verify, "seal_65536": n_seal}
        row, med = _row(_timed(run, tuple(run), reps), items)
        row["n"] = n
        row["hits"] = int(want.sum())
        row["scan_over_verify_per_item"] = {"same_n": round(med["scan"] / med["verify"], 3),
                                            "verify_at_65536": round((med["scan"] / n) / (med["verify_65536"] / n_verify), 3)}
        row["seal_over_verify_per_item_at_65536"] = round(med["seal_65536"] / med["verify_65536"], 3)
        # the A/B: the hooks build of the same sources on the same memos

        def form(env):
            def call():
                for k in AB_ENV:
                    os.environ.pop(k, None)
                os.environ.update(env)
                try:
                    return hctx.note_scan(sks[0], memos_d, leaves_d)[1]
                finally:
                    for k in AB_ENV:
                        os.environ.pop(k, None)
            return call

        ab_run = {name: form(env) for name, env in AB_FORMS}
        for name in ab_run:
            assert np.array_equal(ab_run[name](), want), name
        ab_row, ab_med = _row(_timed(ab_run, tuple(ab_run), reps), {k: n for k in ab_run})
        ab_row["over_shipped"] = {k: round(ab_med[k] / ab_med["shipped"], 3) for k in ab_run if k != "shipped"}
        row["ab_hooks_build"] = ab_row
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del memos_d, notes_d, leaves_d, opened_d, big_d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "note_scan.json"))
    args = ap.parse_args()
    from owshen_amd import api   # (first: it imports torch, whose HIP runtime the libraries then share)
    from owshen_amd import _lib
    from owshen_amd._abi import bind

    hooks = bind(C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libowshen_gpu_hooks.so")))

    class HooksContext(api.Context):
        _lib = hooks

    ctx, hctx = api.Context(0), HooksContext(0)
    out = {"tool": "tools/note_scan_bench.py", "reps": args.reps, "warm_calls": 1, "measured_on_gpu": True, "one_in": ONE_IN,
           "yardstick": "og_eddsa_verify_batch_d on signed records in the same run"}
    tele = None
    try:
        import torch
        from bench import GpuTelemetry, device_identity
        tele = GpuTelemetry(device_identity(torch, ctx.device.index or 0).get("pci"), period=0.02).start()
    except Exception as e:   # the helper is optional
        out["telemetry_error"] = repr(e)[:200]
    out.update(measure(ctx, hctx, [int(s) for s in args.sizes.split(",")], args.reps))
    if tele is not None:
        t = tele.stop() or {}
        out["box"] = {k: t.get(k) for k in ("sclk_MHz", "socket_power_W", "temp_C", "samples", "source")}
    hctx.close()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
