#!/usr/bin/env python3
"""The witness call alone, ONE depth-32 request, of withdraw, transfer, split and join -- --calls times each (default 20) after a warm
call -- for a kernel trace: which part of a call is the three wave-wide launches and which is k_wires_from_limbs.  No counters; a run
of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/split_join_w9_trace.py [--calls 20]

The per-kernel totals of the statistics file divided by --calls + 1 are the time per call (kernel names carry the statement: k_w9_*,
k_tw9_*, k_sw9_*, k_jw9_*; k_wires_from_limbs and the record checks are shared, so --only <statement> traces one statement)."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.join_bench import _join_records  # noqa: E402
from tools.split_join_w9_bench import DEPTH, STATEMENTS, _calls  # noqa: E402
from tools.transfer_bench import _records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=STATEMENTS)
    args = ap.parse_args()
    from owshen_amd import api, circuit
    ctx = api.Context(0)
    for statement in STATEMENTS if args.only is None else (args.only,):
        recs = _join_records(ctx, 1, np.random.default_rng(1)) if statement == "join" else _records(circuit, statement, 1, random.Random(1))
        rec_d = ctx.to_device(recs)
        _prove, witness = _calls(circuit, ctx, statement)
        for _ in range(args.calls + 1):
            witness(rec_d)
        print(statement, "done", flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
