"""The ORDER in which the batched prover issues its work -- every launch, event record, event wait, copy and stream synchronisation,
and the stream each goes to -- against a recording of it (tests/golden/issue_order/*.txt), for every schedule of prove_enqueue.

The CPU interpreter runs every launch to completion when it is issued and ignores hipStreamWaitEvent, so the byte-for-byte emu
cases cannot see a misplaced wait or a kernel on the wrong stream; on the GPU such a mistake may show only under load.  With
HIPEMU_ISSUE_LOG the interpreter writes the issue order down (tests/hipemu/hip/hip_runtime.h), and a change that is meant to leave the
schedule alone must leave this log alone.

The golden files are a RECORDING of the library's behaviour at the commit named in tests/golden/issue_order/README.md; a change that
means to alter the schedule replaces them and says so, a refactor never regenerates them.  The comparison reads both logs the same
way: a record that no later wait in the same log names orders nothing and is dropped; events are then numbered by first appearance
and stream handles (creation numbers of the process) are counted from the context's first stream.
"""
import os
import random

import numpy as np
import pytest

from oracle.py import fields
from tests import groth16_cases as g16_cases, withdraw_cases as wc

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "issue_order")
_SCHED_ENV = ("OG_SUB_BATCH", "OG_PIPE_MIN", "OG_SPLIT_MAX", "OG_ASM_EARLY", "OG_ASM_G2_TREE", "OG_MERGE_LH", "OG_GEN_MIN", "OG_SUB_PLAN",
              "OG_GEN_ONE_SUB", "OG_SUB_CAP", "OG_GLV", "OG_HEAVY", "OG_DEBUG_SYNC")
_WITHDRAW = (2, 2, 3)   # depth, n_pad3, n_pad2
# the withdraw cases walk their MiMC7 chains in the lane-local kernels: every cross-lane read of the wave-wide walk is a rendezvous of
# the whole workgroup on the interpreter, and which witness kernel runs is not what these cases are about
_QUICK_WALK = {"OG_WITNESS_W9": "0"}


def normalise(text):
    """the log as a list of lines: dead records dropped, events renumbered by first appearance, streams relative to the first one"""
    rows = [ln.split() for ln in text.splitlines() if ln.strip()]
    base = min(int(r[1]) for r in rows if int(r[1]) > 0) - 1
    waited_later, keep = set(), []
    for r in reversed(rows):
        if r[0] == "W":
            waited_later.add(r[2])
        if r[0] == "R":
            if r[2] not in waited_later:
                continue
            waited_later.discard(r[2])   # (a later wait refers to THIS record: an earlier record of the event needs a wait of its own)
        keep.append(r)
    keep.reverse()
    names, out = {}, []
    for r in keep:
        r = list(r)
        if int(r[1]) > 0:
            r[1] = str(int(r[1]) - base)
        if r[0] in "RW":
            r[2] = str(names.setdefault(r[2], len(names)))
        out.append(" ".join(r))
    return out


@pytest.fixture(scope="module")
def world():
    from tests import emu
    from owshen_amd import circuit, groth16 as g16
    from tests.r1cs_util import random_r1cs
    ctx = emu.Ctx()

    def toy_case(n_proofs):   # (the shape of test_emu_multi8.py's toy case)
        n_wires, cons, z0 = random_r1cs(6, 1, seed=8)
        blob, _vk = g16.setup(ctx, g16.R1CS.from_constraints(n_wires, 1, cons), 3, 5, 7, 11, 13)
        zs = []
        for t in range(n_proofs):
            z, r2 = list(z0), random.Random(700 + t)
            for i in range(1, n_wires - len(cons)):
                z[i] = r2.randrange(fields.R)
            for k, (a, b, _c) in enumerate(cons):
                z[n_wires - len(cons) + k] = sum(v * z[i] for i, v in a.items()) * sum(v * z[i] for i, v in b.items()) % fields.R
            zs.append(np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(-1, 32))
        return blob, np.stack(zs)

    w = {"ctx": ctx, "proofs": {}}
    w["blob"], w["zs"], w["rs"] = g16_cases.medium_case(ctx, 60, 9)   # (the circuit of case_medium_circuit_vs_c_oracle)
    w["pk"] = g16.ProvingKey(ctx, w["blob"])
    blob6, w["zs6"] = toy_case(3)
    w["pk6"] = g16.ProvingKey(ctx, blob6)
    w["wpk"] = wc._key(ctx, *_WITHDRAW)[3]
    rnd = random.Random(31)
    w["recs"] = [ctx.to_device(np.stack([wc._pack(circuit, wc._inputs(rnd, _WITHDRAW[0])) for _ in range(3)])) for _call in range(2)]
    w["wrs"] = [[(rnd.randrange(fields.R), rnd.randrange(fields.R)) for _ in range(3)] for _call in range(2)]
    yield w
    ctx.close()


def _prove(w, n, device=True):
    """n proofs of the 60-constraint circuit; whatever the schedule, proof k is the same bytes"""
    pk, zs, rs = w["pk"], w["zs"][:n], w["rs"][:n]
    got = pk.prove_batch_device(w["ctx"].to_device(zs), rs) if device else pk.prove_batch(zs, rs)
    for k in range(n):
        assert w["proofs"].setdefault(k, got[k].tobytes()) == got[k].tobytes(), f"proof {k} differs between two schedules"


def _fan_out_2(w): _prove(w, 2)
def _fan_out_3(w): _prove(w, 3)
def _sym_5(w): _prove(w, 5)
def _pipe_9(w): _prove(w, 9)
def _host_witnesses_5(w): _prove(w, 5, device=False)


def _one_stream_5(w):
    w["ctx"].set_lanes(1)
    try:
        _prove(w, 5)
    finally:
        w["ctx"].set_lanes(2)


def _two_calls_in_flight(w):
    from owshen_amd import circuit
    jobs = [circuit.submit_from_inputs(w["ctx"], w["wpk"], _WITHDRAW[0], w["recs"][c], w["wrs"][c], *_WITHDRAW[1:], return_public=True)
            for c in range(2)]
    for j in jobs:
        j.wait()


def _sharded_front(w):
    w["pk6"].prove_partials_device(w["ctx"].to_device(w["zs6"]), 1, 2)


def _host_chains_2(w):
    from owshen_amd import circuit
    w["ctx"].set_host_chains(8)
    try:
        circuit.prove_from_inputs(w["ctx"], w["wpk"], _WITHDRAW[0], w["recs"][0][:2], w["wrs"][0][:2], *_WITHDRAW[1:], return_public=True)
    finally:
        w["ctx"].set_host_chains(0)


CASES = {
    "fan_out_2": ({}, _fan_out_2),                                                        # two-part assembly, the G2 half as a tree
    "fan_out_3_one_part": ({"OG_ASM_EARLY": "0", "OG_ASM_G2_TREE": "0"}, _fan_out_3),
    "sym_5": ({"OG_SPLIT_MAX": "1"}, _sym_5),                                             # 3 + 2 side by side on the two lanes
    "pipe_9_merged": ({"OG_SUB_BATCH": "2", "OG_PIPE_MIN": "1", "OG_MERGE_LH": "1"}, _pipe_9),   # plan 1, 2, 2, 2, 2: slots are reused
    "pipe_9_apart": ({"OG_SUB_BATCH": "2", "OG_PIPE_MIN": "1", "OG_MERGE_LH": "0"}, _pipe_9),
    "pipe_two_calls_gen": ({"OG_SUB_BATCH": "2", "OG_PIPE_MIN": "1", "OG_GEN_MIN": "1", **_QUICK_WALK}, _two_calls_in_flight),
    "one_stream_5": ({"OG_SUB_BATCH": "2"}, _one_stream_5),
    "host_witnesses_5": ({"OG_SUB_BATCH": "2"}, _host_witnesses_5),
    "sharded_front_rank1_of_2": ({}, _sharded_front),
    "host_chains_2": (_QUICK_WALK, _host_chains_2),
}


def record(w, name, path, monkeypatch):
    """run the case with the interpreter's issue log in `path`; returns the raw log"""
    env, call = CASES[name]
    for k in _SCHED_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    saved = w["pk"]
    if "OG_MERGE_LH" in env:   # (read when a key is loaded: these cases load their own)
        from owshen_amd import groth16 as g16
        w["pk"] = g16.ProvingKey(w["ctx"], w["blob"])
    try:
        # The log must not depend on what the context did before.  A first, unlogged run grows the scratch arena to what the case
        # needs (growing it drains the streams); a blocking call that fans out then leaves the context behind a call that did not
        # go through the stage pipeline, all streams idle.
        call(w)
        w["pk6"].prove_batch(w["zs6"][:1], [(1, 2)])
        monkeypatch.setenv("HIPEMU_ISSUE_LOG", path)
        try:
            call(w)
        finally:
            monkeypatch.delenv("HIPEMU_ISSUE_LOG")
    finally:
        if w["pk"] is not saved:
            w["pk"].close()
            w["pk"] = saved
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize("name", list(CASES))
def test_emu_issue_order_is_the_recorded_one(world, name, tmp_path, monkeypatch):
    got = normalise(record(world, name, str(tmp_path / "issue.log"), monkeypatch))
    with open(os.path.join(_GOLDEN, name + ".txt")) as f:
        want = normalise(f.read())
    for k in range(max(len(got), len(want))):
        if k >= len(got) or k >= len(want) or got[k] != want[k]:
            ctx_lines = "\n".join(f"  {j + 1:6d}  recorded: {want[j] if j < len(want) else '<end>':60s} now: {got[j] if j < len(got) else '<end>'}"
                                  for j in range(max(0, k - 5), min(max(len(got), len(want)), k + 6)))
            pytest.fail(f"{name}: the issue order differs from the recording at line {k + 1} ({len(want)} recorded, {len(got)} now)\n{ctx_lines}")
