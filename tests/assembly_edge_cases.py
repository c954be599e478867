"""The proof assembly (owshen_amd/csrc/ecmul_impl.hip.h, groth16.hip) at the edges of the blinding pair (r, s), in every form, through the
public proving calls -- TEST INFRASTRUCTURE ONLY; tests/test_emu_assembly_edge.py runs it on the CPU interpreter (a reduced scalar
list that still covers every class below and every form) and tests/test_gpu_assembly_edge.py on the hardware (the whole list).

Circuit random_r1cs(12, 2, seed): domain 16.  Three keys from the product's own groth16.setup:
  K0   random toxic values, three witnesses;
  Ka   alpha = -sum z_i a_i(tau) for one fixed witness z: alpha + A is the point at infinity (the `p.is_inf()` exit of the wave-wide
       kernel, an infinite base in the others), and with r = 0 the proof's A is itself infinity (xyzz_to_affine with ZZ = 0);
  Kb   beta = -sum z_i b_i(tau): beta + B1 and beta2 + B2 are infinity, and with s = 0 so is the proof's B.
Expected bytes: the C restatement for every proof, oracle/py/groth16.prove for the first twelve of a key and every special pair;
the product's verifier accepts every K0 proof (World.verify_k0, on the bytes every form must return).

Scalars (SCALARS below), each as r beside a random s, as s beside a random r, and as the product r s; r = s; (r, 0); (0, s); (0, 0);
r s = 1.  The library rounds its GLV decomposition down, so WHICH halves a scalar gives is asked of og_glv_decompose, and
`coverage` asserts that the halves the library itself forms hit every class -- a zero half, each sign combination it can form (the
first half is never negative: see CLASSES), a half of 2^126 and more, a half whose top eight windows are empty -- in each of the
three positions (r, r s, s) the assembly decomposes.

Forms (FORMS below): the four products by a wave per half (w9), a lane per half (glv) or a lane per 254-bit scalar (plain), each in
two parts with the G2 tree (the fanned-out call) and in one part with a lane per proof in G2 (one stream, or the hooks build's
switches), and the host assembly.  A form is confirmed by og_prove_plan, by the number of timed assembly regions (three: B's half,
the products and A, C; two or one in one part; on the host the one empty region where B's half would be) and, on the interpreter, by the kernels its issue log names.

Non-canonical pairs (R, R + 7, 2^256 - 1 in either slot): the contract include/owshen_gpu.h states -- the proof of (r mod R, s mod R)."""
import ctypes as C
import random

import numpy as np

from oracle.py import fields, groth16 as og16
from tests.r1cs_util import random_r1cs, oracle_c_key_from_blob

R = fields.R
LAM = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd      # tests/test_glv.py derives it from the moduli
N_CONSTRAINTS, N_PUB, SEED = 12, 2, 1212
TOXIC0 = (0x1234567 ** 5 % R, 0x7654321 ** 6 % R, 0x1122334 ** 7 % R, 0x5566778 ** 8 % R, 0x99aabbc ** 9 % R)
NONCANONICAL = (R, R + 7, (1 << 256) - 1)


def _halves_scalars():
    big1, big2 = (1 << 126) + 0x1234567, (1 << 126) + (1 << 125) + 0x7654321
    shapes = [(big1, big2), ((1 << 127) - 1, (1 << 124) - 1), ((1 << 124) - 1, (1 << 127) - 1),       # halves >= 2^126; every nibble 0xF
              (5, 9), (3 << 124, 6 << 124), (0xF, 7 << 124), (7 << 124, 0xF),                          # one nibble, window 0 | 31
              (1, big2), (big1, 1), (1, 1), (0, big1), (0, 1), (0, 3 << 124)]                          # a half of 1; k1 = 0 (k2 = 0 is the small scalars)
    out = []
    for k1, k2 in shapes:
        for s1 in (1, -1):
            for s2 in (1, -1):
                if (s1 < 0 and k1 == 0) or (s2 < 0 and k2 == 0):
                    continue
                out.append((s1 * k1 + LAM * s2 * k2) % R)
    return out


SCALARS = [0, 1, 2, 15, 16, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 127) - 1, 1 << 127, (1 << 128) - 1, 1 << 253,
           LAM, LAM + 1, LAM - 1, R - LAM] + [m * LAM % R for m in range(2, 17)] + _halves_scalars()
# k1 is never negative: with both quotients rounded DOWN the halves are f1 (a1, b1) + f2 (a2, b2) with f1, f2 in [0, 1), and a1, a2 > 0
# (glv.h), so k1 = f1 a1 + f2 a2 >= 0 and only k2 takes either sign -- the sign combinations "-+" and "--" cannot be formed through
# any public call, and classes_of asserts that none is (a decomposition that rounds to nearest would trip it and has to add them here)
CLASSES = ("zero", "++", "+-", "big", "short")
POSITIONS = ("r", "rs", "s")


def glv_halves(lib, k):
    """the halves (k1, k2) the LIBRARY forms for a canonical k (og_glv_decompose)"""
    out = (C.c_uint8 * 32)()
    rc = lib.og_glv_decompose((C.c_uint8 * 32).from_buffer_copy(int(k).to_bytes(32, "little")), out)
    assert rc == 0, k
    hs = []
    for h in (bytes(out)[:16], bytes(out)[16:]):
        v = int.from_bytes(h, "little")
        hs.append(-(v & ((1 << 127) - 1)) if v >> 127 else v)
    assert (hs[0] + LAM * hs[1] - k) % R == 0
    return tuple(hs)


def classes_of(halves):
    k1, k2 = halves
    assert k1 >= 0, "a negative first half: the sign classes of this module no longer cover what the library forms"
    out = set()
    if k1 == 0 or k2 == 0:
        out.add("zero")
    if k1 and k2:
        out.add(("-" if k1 < 0 else "+") + ("-" if k2 < 0 else "+"))
    if max(abs(k1), abs(k2)) >= 1 << 126:
        out.add("big")
    if any(h and abs(h) < 1 << 96 for h in halves):
        out.add("short")
    return out


def pair_classes(lib, pair):
    """{(position, class)} of a canonical pair"""
    r, s = pair
    return {(pos, c) for pos, k in zip(POSITIONS, (r, r * s % R, s)) for c in classes_of(glv_halves(lib, k))}


def all_pairs(lib):
    """the whole list: [(tag, (r, s))]"""
    rnd = random.Random("assembly_edge/pairs")
    rand = lambda: rnd.randrange(1, R)
    pairs = [("zero-zero", (0, 0)), ("r-zero", (rand(), 0)), ("zero-s", (0, rand())), ("r-eq-s", (rand(),) * 2), ("r-eq-s-lam", (LAM, LAM)),
             ("r-eq-s-top", (R - 1, R - 1))]
    r1 = rand()
    pairs.append(("rs-one", (r1, pow(r1, -1, R))))
    for k in SCALARS:
        pairs.append((f"r={k:#x}", (k, rand())))
        pairs.append((f"s={k:#x}", (rand(), k)))
        r0 = rand()
        pairs.append((f"rs={k:#x}", (r0, k * pow(r0, -1, R) % R)))
    # the library's own halves must hit every class in every position: search deterministic candidates for what is still missing
    need = {(p, c) for p in POSITIONS for c in CLASSES}
    for _t, p in pairs:
        need -= pair_classes(lib, p)
    t = 0
    while need and t < 4096:
        t += 1
        k = (t * 0x9E3779B97F4A7C15 + (LAM * (t * t + 1) << (t % 120))) % R
        for cand in ((k, 1 + t), (1 + t, k), (1 + t, k * pow(1 + t, -1, R) % R)):
            got = pair_classes(lib, cand) & need
            if got:
                pairs.append((f"search-{t}", cand))
                need -= got
    assert not need, f"no pair whose library halves are {sorted(need)}"
    assert all(r * s % R == 0 for _t, (r, s) in pairs[:3]) and pairs[6][1][0] * pairs[6][1][1] % R == 1
    return pairs


def coverage(lib, pairs):
    """every class in every position, by the halves the library forms; -> {(position, class): count}"""
    count = {(p, c): 0 for p in POSITIONS for c in CLASSES}
    for _t, pair in pairs:
        for key in pair_classes(lib, pair):
            count[key] += 1
    missing = sorted(k for k, v in count.items() if v == 0)
    assert not missing, f"no pair whose library halves are {missing}"
    return count


def reduced_pairs(lib, pairs):
    """a greedy cover of every (position, class) plus the special pairs: what the CPU interpreter's twin proves"""
    keep = list(pairs[:7])
    need = {(p, c) for p in POSITIONS for c in CLASSES}
    for _t, p in keep:
        need -= pair_classes(lib, p)
    rest = list(pairs[7:])
    while need:
        best = max(rest, key=lambda tp: len(pair_classes(lib, tp[1]) & need))
        got = pair_classes(lib, best[1]) & need
        assert got
        keep.append(best)
        need -= got
        rest.remove(best)
    coverage(lib, keep)
    return keep


def _wit(z):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in z), dtype=np.uint8).reshape(-1, 32).copy()


class Key:
    pass


class World:
    """the circuit, the three keys (product blob, resident key, C restatement, oracle/py key) and the expected bytes, built once per context"""

    def __init__(self, ctx):
        from owshen_amd import groth16 as g16
        self.ctx, self.g16 = ctx, g16
        n_wires, cons, z0 = random_r1cs(N_CONSTRAINTS, N_PUB, seed=SEED)
        self.ro = og16.R1CS(n_wires, N_PUB, cons)
        assert self.ro.domain_size == 16
        r1 = g16.R1CS.from_constraints(n_wires, N_PUB, cons)
        zs = [list(z0)]
        for t in (1, 2):
            z, r2 = list(z0), random.Random(SEED + t)
            for i in range(1, n_wires - len(cons)):
                z[i] = r2.randrange(R)
            for k, (a, b, _c) in enumerate(cons):
                z[n_wires - len(cons) + k] = sum(v * z[i] for i, v in a.items()) * sum(v * z[i] for i, v in b.items()) % R
            assert self.ro.is_satisfied(z)
            zs.append(z)
        tau = TOXIC0[0]
        qa, qb, _qc, _z = og16.qap_at(self.ro, tau)
        alpha = -sum(z * a for z, a in zip(z0, qa)) % R
        beta = -sum(z * b for z, b in zip(z0, qb)) % R
        assert 0 < alpha < R and 0 < beta < R
        self.keys = {}
        for name, toxic, wits in (("K0", TOXIC0, zs), ("Ka", (tau, alpha) + TOXIC0[2:], zs[:1]), ("Kb", (tau, TOXIC0[1], beta) + TOXIC0[3:], zs[:1])):
            k = Key()
            k.name, k.toxic, k.zs = name, toxic, wits
            k.blob, k.vk = g16.setup(ctx, r1, *toxic)
            k.pk = g16.ProvingKey(ctx, k.blob)
            k.ck = oracle_c_key_from_blob(k.blob)
            k.pk_o = None
            k.want = {}
            self.keys[name] = k
        self.pairs = all_pairs(ctx._lib)
        self.cover = coverage(ctx._lib, self.pairs)

    def witness(self, key, j):
        return self.keys[key].zs[j % len(self.keys[key].zs)]

    def expected(self, key, j, pair):
        """the C restatement's bytes for witness j of the key and the pair reduced mod R (computed once)"""
        k = self.keys[key]
        r, s = pair[0] % R, pair[1] % R
        slot = (j % len(k.zs), r, s)
        if slot not in k.want:
            k.want[slot] = k.ck.prove(_wit(self.witness(key, j)), r, s)
        return k.want[slot]

    def oracle_py(self, key, j, pair):
        k = self.keys[key]
        if k.pk_o is None:
            k.pk_o, k.vk_o = og16.setup(self.ro, *k.toxic)
        return og16.proof_to_bytes(og16.prove(k.pk_o, self.ro, self.witness(key, j), pair[0] % R, pair[1] % R))

    def verify_k0(self, pairs, batched):
        """the verifier accepts the proof of every pair under K0 -- the bytes `expected` holds, which run_form demands of every form;
        batched: one og_verify_batch_d call (the GPU), else og_verify proof by proof (the interpreter's handful)"""
        k, g16 = self.keys["K0"], self.g16
        vkb = g16.vk_to_bytes(k.vk)
        proofs = [self.expected("K0", j, pair) for j, (_t, pair) in enumerate(pairs)]
        pubs = [self.witness("K0", j)[1:N_PUB + 1] for j in range(len(pairs))]
        if batched:
            with g16.VerifyingKey(self.ctx, vkb) as vk:
                ok = vk.verify_batch(np.stack([_wit(p) for p in pubs]), np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(-1, 256).copy())
        else:
            ok = [g16.verify(vkb, pub, proof, lib=self.ctx._lib) for pub, proof in zip(pubs, proofs)]
        bad = [pairs[i][0] for i, v in enumerate(ok) if not v]
        assert not bad and len(ok) == len(pairs), f"K0 proofs the verifier rejects: {bad}"
        return len(ok)

    def close(self):
        for k in self.keys.values():
            k.pk.close()
        _WORLDS.pop(id(self.ctx), None)


_WORLDS = {}


def world(ctx):
    if id(ctx) not in _WORLDS:
        _WORLDS[id(ctx)] = World(ctx)
    return _WORLDS[id(ctx)]


# form -> (environment of the hooks build, lanes, host chains, chunk, expected plan, assembly regions, kernels the call must / must not launch)
_TWO = ("k_assemble_g1_early", "k_assemble_g1_late", "k_assemble_g2_tree")
_ONE = ("k_assemble_g1_finish", "k_assemble_g2")
_MULS = ("k_assemble_g1_muls_w9", "k_assemble_g1_muls_glv", "k_assemble_g1_muls")
_ONE_ENV = {"OG_ASM_EARLY": "0", "OG_ASM_G2_TREE": "0"}
FORMS = {
    "w9/two-part":          dict(env={}, lanes=2, host=0, chunk=8, plan="query fan-out", regions=3, muls="k_assemble_g1_muls_w9", parts=_TWO),
    "w9/one-part":          dict(env=_ONE_ENV, lanes=2, host=0, chunk=8, plan="query fan-out", regions=2, muls="k_assemble_g1_muls_w9", parts=_ONE),
    "w9/one-stream":        dict(env={}, lanes=1, host=0, chunk=8, plan="serial", regions=1, muls="k_assemble_g1_muls_w9", parts=_ONE),
    "glv/two-part":         dict(env={"OG_ASM_W9_MAX": "0"}, lanes=2, host=0, chunk=8, plan="query fan-out", regions=3, muls="k_assemble_g1_muls_glv", parts=_TWO),
    "glv/two-part/9..64":   dict(env={}, lanes=2, host=0, chunk=64, plan="query fan-out", regions=3, muls="k_assemble_g1_muls_glv", parts=_TWO),
    "glv/one-part":         dict(env=dict(_ONE_ENV, OG_ASM_W9_MAX="0"), lanes=2, host=0, chunk=8, plan="query fan-out", regions=2, muls="k_assemble_g1_muls_glv", parts=_ONE),
    "glv/one-stream/9..64": dict(env={}, lanes=1, host=0, chunk=64, plan="serial", regions=1, muls="k_assemble_g1_muls_glv", parts=_ONE),
    "plain/two-part":       dict(env={"OG_GLV": "0"}, lanes=2, host=0, chunk=8, plan="query fan-out", regions=3, muls="k_assemble_g1_muls", parts=_TWO),
    "plain/two-part/65..":  dict(env={}, lanes=2, host=0, chunk=96, plan="query fan-out", regions=3, muls="k_assemble_g1_muls", parts=_TWO),
    "plain/one-part":       dict(env=dict(_ONE_ENV, OG_GLV="0"), lanes=2, host=0, chunk=8, plan="query fan-out", regions=2, muls="k_assemble_g1_muls", parts=_ONE),
    "plain/one-stream/65..": dict(env={}, lanes=1, host=0, chunk=96, plan="serial", regions=1, muls="k_assemble_g1_muls", parts=_ONE),
    "host":                 dict(env={}, lanes=2, host=8, chunk=8, plan="query fan-out", regions=1, muls=None, parts=()),
}
_ENV_NAMES = ("OG_GLV", "OG_ASM_W9_MAX", "OG_ASM_EARLY", "OG_ASM_G2_TREE")


def _chunks(items, size, least):
    """consecutive calls of at most `size` proofs and at least `least` (the last call takes what is left of the one before it)"""
    out = [items[i:i + size] for i in range(0, len(items), size)]
    if len(out) > 1 and len(out[-1]) < least:
        tail = out.pop()
        out[-1] = out[-1] + tail
        if len(out[-1]) > size:
            both = out.pop()
            out += [both[:len(both) // 2], both[len(both) // 2:]]
    return out


def launches_of(path):
    """kernel names of an interpreter issue log"""
    with open(path) as f:
        return [row[2] for row in (ln.split() for ln in f) if row and row[0] == "L"]


def run_form(ctx, monkeypatch, form, key, pairs, issue_log=None, check_py=0, noncanonical=False):
    """prove `pairs` ([(tag, (r, s))]) under the key in the form; every proof against the C restatement; -> (proofs, calls).
    A call below the form's natural size is filled up with repeats of its first pairs (a 9..64 or 65.. form needs its count)."""
    w, f = world(ctx), FORMS[form]
    k = w.keys[key]
    least = {8: 1, 64: 9, 96: 65}[f["chunk"]]
    for name in _ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, v in f["env"].items():
        monkeypatch.setenv(name, v)
    if least == 1 and "OG_ASM_W9_MAX" not in f["env"]:
        monkeypatch.setenv("OG_ASM_W9_MAX", "8")      # (tests/emu.py sets 0 for the interpreter's other cases; 8 is the library's default)
    ctx.set_lanes(f["lanes"])
    ctx.set_host_chains(f["host"])
    n_proofs = n_calls = 0
    try:
        items = list(enumerate(pairs))
        while len(items) < least:
            items = items + items[:least - len(items)]
        for call in _chunks(items, f["chunk"], least):
            n = len(call)
            assert least <= n <= f["chunk"]
            wits = np.stack([_wit(w.witness(key, j)) for j, _tp in call])
            rs = [tp[1] for _j, tp in call]
            assert k.pk.plan(n) == (f["plan"], [n]), (form, k.pk.plan(n))
            ctx.profile(True)
            if issue_log:
                open(issue_log, "w").close()
                monkeypatch.setenv("HIPEMU_ISSUE_LOG", issue_log)
            try:
                got = k.pk.prove_batch(wits, rs)
            finally:
                if issue_log:
                    monkeypatch.delenv("HIPEMU_ISSUE_LOG")
            regions = ctx.profile_read()["assemble"]
            ctx.profile(False)
            assert regions[1] == f["regions"] and regions[2] == (0 if f["host"] else n), (form, regions)
            if issue_log:
                names = launches_of(issue_log)
                muls = f["muls"] and (_MULS[2] if noncanonical else f["muls"])     # one non-canonical scalar: the whole call walks 256 bits
                for kern in _MULS + _TWO + _ONE:
                    want = 1 if kern == muls or kern in f["parts"] else 0
                    assert names.count(kern) == want, f"{form}: {kern} launched {names.count(kern)} times, expected {want}"
            for (j, (tag, pair)), proof in zip(call, got):
                assert noncanonical or (pair[0] < R and pair[1] < R)
                where = f"{form} key {key} witness {j % len(k.zs)} pair {tag}"
                assert proof.tobytes() == w.expected(key, j, pair), f"{where}: not the restatement's bytes (which verify: World.verify_k0)"
                n_proofs += 1
            n_calls += 1
        for j, (tag, pair) in list(enumerate(pairs))[:check_py]:
            assert w.expected(key, j, pair) == w.oracle_py(key, j, pair), f"key {key} pair {tag}: the two oracles differ"
    finally:
        ctx.set_lanes(2)
        ctx.set_host_chains(0)
    return n_proofs, n_calls


def infinity_checks(ctx):
    """what the edge keys are for, seen in the expected bytes themselves: A is 64 zero bytes under Ka with r = 0, B is 128 zero bytes
    under Kb with s = 0, and neither under K0"""
    w = world(ctx)
    assert w.expected("Ka", 0, (0, 5))[:64] == bytes(64) and w.expected("Ka", 0, (1, 5))[:64] != bytes(64)
    assert w.expected("Kb", 0, (5, 0))[64:192] == bytes(128) and w.expected("Kb", 0, (5, 1))[64:192] != bytes(128)
    assert w.expected("K0", 0, (0, 0))[:64] != bytes(64) and w.expected("K0", 0, (0, 0))[64:192] != bytes(128)
    # with alpha + A at infinity, A = r delta whatever the witness part was
    from oracle.py.curve import G1, G1_GEN, g1_to_bytes
    assert w.expected("Ka", 0, (7, 5))[:64] == g1_to_bytes(G1.mul(G1_GEN, 7 * w.keys["Ka"].toxic[4] % R))


def edge_key_pairs(pairs):
    """the special pairs and the first scalars of the list in each position: what the edge keys Ka and Kb prove (with the infinities)"""
    return pairs[:7] + pairs[7:7 + 3 * 8]


def noncanonical_pairs():
    rnd = random.Random("assembly_edge/noncanonical")
    out = []
    for v in NONCANONICAL:
        out.append((f"r={v:#x}", (v, rnd.randrange(1, R))))
        out.append((f"s={v:#x}", (rnd.randrange(1, R), v)))
    out.append(("both", (NONCANONICAL[1], NONCANONICAL[2])))
    return out
