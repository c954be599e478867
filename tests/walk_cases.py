"""Cases for the two walks of the split and the join statement, shared by the CPU-interpreter run and the GPU run: the lane-local
kernels (k_split_core, k_join_core) and the wave-wide walk (k_sw9_*, k_jw9_*: one permutation per one-wave workgroup in three
launches) against the plain restatements in tests/split_spec.py and tests/join_spec.py; the launches of one witness call from the
interpreter's issue log; and a join request whose two paths do not meet, on the wave-wide walk."""
import random

import numpy as np
import pytest

from oracle.py import fields, mimc7
from tests import join_cases, split_cases
from tests.transfer_cases import LANE_LOCAL, walk  # noqa: F401  (LANE_LOCAL: for the callers)

R = fields.R
STATEMENTS = {"split": split_cases, "join": join_cases}
EDGE_COUNT = {"split": 3, "join": 5}     # how many requests of edge_inputs are edges by construction
_wit_bytes = join_cases._wit_bytes       # (statement-independent: a list of integers -> [1, n_wires, 32] bytes)


def witness(circuit, statement):
    return getattr(circuit, statement + "_witness")


def prove(circuit, statement):
    return getattr(circuit, statement + "_prove")


def edge_requests(statement, rnd, depth, n):
    """the first n of the statement's edge requests, random well-formed ones behind them"""
    return STATEMENTS[statement].edge_inputs(rnd, depth, max(n, EDGE_COUNT[statement]))[:n]


def pack(statement, ins):
    from owshen_amd import circuit
    return np.stack([STATEMENTS[statement]._pack(circuit, i) for i in ins])


def spec_bytes(statement, depth, ins):
    """the spec's witnesses of `ins`: what every walk must return, byte for byte"""
    return np.concatenate([_wit_bytes(STATEMENTS[statement]._spec(i, depth)[3]) for i in ins]).tobytes()


def case_walks_agree(ctx, statement, depth, ins, want=None):
    """the lane-local walk and the wave-wide walk in each of its three round forms, forced through OG_WITNESS_W9 / OG_W9_ROWS and
    chosen through OG_WITNESS_W9_MAX at n - 1 (lane-local) and at n (wave-wide): the spec's bytes every time.  `ctx` reads the hooks."""
    from owshen_amd import circuit
    n = len(ins)
    recs = pack(statement, ins)
    want = spec_bytes(statement, depth, ins) if want is None else want
    settings = [dict(OG_WITNESS_W9=0)] + [dict(OG_WITNESS_W9=1, OG_W9_ROWS=rows) for rows in (0, 1, 2)]
    settings += [dict(OG_WITNESS_W9_MAX=n - 1), dict(OG_WITNESS_W9_MAX=n)]
    for env in settings:
        with walk(**env):
            got = ctx.to_host(witness(circuit, statement)(ctx, depth, ctx.to_device(recs)))
        if got.tobytes() != want:
            w = np.frombuffer(want, dtype=np.uint8).reshape(got.shape)
            bad = np.argwhere((got != w).any(axis=2))
            raise AssertionError(f"{statement} depth {depth}, {env}: {len(bad)} wires differ, the first (request, wire) = {tuple(bad[0])}")


def launches(ectx, statement, depth, n, tmp_path, monkeypatch, **env):
    """(kernel, grid, block) of every launch of one og_<statement>_witness_d call of n requests, from HIPEMU_ISSUE_LOG"""
    from owshen_amd import circuit
    rnd = random.Random(60 + n)
    recs = ectx.to_device(pack(statement, edge_requests(statement, rnd, depth, n)))
    path = str(tmp_path / ("issue_" + "_".join(f"{k}_{v}" for k, v in sorted(env.items())) + ".log"))   # (the log is appended to)
    with walk(**env):
        witness(circuit, statement)(ectx, depth, recs)          # (unlogged: grows the scratch arena to what the call needs)
        monkeypatch.setenv("HIPEMU_ISSUE_LOG", path)
        try:
            witness(circuit, statement)(ectx, depth, recs)
        finally:
            monkeypatch.delenv("HIPEMU_ISSUE_LOG")
    out = []
    with open(path) as f:
        for row in (ln.split() for ln in f):
            if row and row[0] == "L":
                out.append((row[2], tuple(int(x) for x in row[3].split(",")), int(row[4])))
    return out


def foreign_join_request(rnd, depth):
    """(request, note a's root): a well-formed join record whose note b has a foreign top sibling, so that the two paths do not meet
    (tests/join_cases.py case_different_roots); the root is the spec's walk of note a"""
    i = join_cases._inputs(rnd, depth)
    foreign = dict(i, siblings_b=i["siblings_b"][:-1] + [rnd.randrange(R)])
    root_a = mimc7.merkle_root_from_path(join_cases._leaf(i, "a"), i["index_a"], i["siblings_a"])[-1]
    assert mimc7.merkle_root_from_path(join_cases._leaf(i, "b"), foreign["index_b"], foreign["siblings_b"])[-1] != root_a
    return foreign, root_a


def case_join_paths_do_not_meet(ctx, depth, key=None, seed=7):
    """under the FORCED wave-wide walk: wire 1 is note a's root -- note b's chain block stores nothing for its last level -- every
    other wire of note b's walk is what the lane-local walk stores, and og_join_prove_batch_d answers OG_ERR_UNSATISFIED"""
    from owshen_amd import api, circuit
    rnd = random.Random(seed * 1000 + depth)
    foreign, root_a = foreign_join_request(rnd, depth)
    rec = pack("join", [foreign])
    blob, vk, pk, close = key if key is not None else join_cases._key(ctx, depth)
    with walk(OG_WITNESS_W9=1):
        wit = ctx.to_host(circuit.join_witness(ctx, depth, ctx.to_device(rec)))
        assert api.bytes_to_ints(wit[0][1:2]) == [root_a]
        with pytest.raises(api.OwshenGpuError) as e:
            circuit.join_prove(ctx, pk, depth, ctx.to_device(rec), [(rnd.randrange(R), rnd.randrange(R))])
        assert e.value.code == -4, str(e.value)
    with walk(**LANE_LOCAL):
        assert ctx.to_host(circuit.join_witness(ctx, depth, ctx.to_device(rec))).tobytes() == wit.tobytes()
    close()
