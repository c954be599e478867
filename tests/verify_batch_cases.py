"""Batched Groth16 verification on the device (og_vk_load / og_verify_batch_d, owshen_amd/csrc/verify_gpu.hip) against og_verify,
proof by proof; shared by the CPU-interpreter run and the GPU run.

The expected answer of EVERY entry is og_verify's own (owshen_amd.verify_only: the host-only library), and for the well-formed
entries also the Python oracle's pairing check (oracle/py/groth16.py).  og_verify_batch_d takes the number of public inputs
from the key handle: a batch whose n_pub differs from the key's cannot be expressed at this interface, so og_verify's "number
of public inputs does not match" has no counterpart here."""
import ctypes as C
import hashlib
import random
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle.py import fields, groth16 as og16
from oracle.py.curve import G1, G2, g1_to_bytes, g2_to_bytes
from tests.r1cs_util import random_r1cs

R, P = fields.R, fields.P


def _le(v):
    return int(v).to_bytes(32, "little")


def vk_blob(vk):
    return (b"OWVK0001" + struct.pack("<Q", len(vk["ic"]) - 1) + g1_to_bytes(vk["alpha_g1"]) + g2_to_bytes(vk["beta_g2"]) +
            g2_to_bytes(vk["gamma_g2"]) + g2_to_bytes(vk["delta_g2"]) + b"".join(g1_to_bytes(p) for p in vk["ic"]))


class Instance:
    """a random R1CS with n_pub public inputs, its keys, and proofs of as many witnesses as asked for"""

    def __init__(self, n_pub, seed):
        self.n_pub = n_pub
        self.n_wires, self.cons, self.z0 = random_r1cs(9, n_pub, seed=seed)
        self.r1cs = og16.R1CS(self.n_wires, n_pub, self.cons)
        self.rnd = random.Random(seed * 7 + 1)
        self.pk, self.vk = og16.setup(self.r1cs, *(self.rnd.randrange(1, R) for _ in range(5)))
        self.blob = vk_blob(self.vk)
        self.n_in = self.n_wires - len(self.cons)

    def witness(self, inputs):
        """the witness that starts with `inputs` (public, then free): every constraint defines its own product wire"""
        z = [1] + [int(v) % R for v in inputs]
        assert len(z) == self.n_in
        for a, b, _c in self.cons:
            z.append(sum(v * z[i] for i, v in a.items()) % R * (sum(v * z[i] for i, v in b.items()) % R) % R)
        assert self.r1cs.is_satisfied(z)
        return z

    def prove(self, inputs=None):
        z = self.z0 if inputs is None else self.witness(inputs)
        proof = og16.proof_to_bytes(og16.prove(self.pk, self.r1cs, z, self.rnd.randrange(R), self.rnd.randrange(R)))
        return [int(v) for v in z[1:1 + self.n_pub]], proof


def _fq2_sqrt(a):
    """a square root of a in Fq2 = Fq[u]/(u^2 + 1), or None (p = 3 mod 4)"""
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (P + 1) // 4, P)
        if s * s % P == a0:
            return (s, 0)
        s = pow(-a0 % P, (P + 1) // 4, P)
        return (0, s) if s * s % P == -a0 % P else None
    n = (a0 * a0 + a1 * a1) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return None
    for sg in (s, -s % P):
        h = (a0 + sg) * pow(2, -1, P) % P
        x0 = pow(h, (P + 1) // 4, P)
        if x0 * x0 % P == h and x0:
            return (x0, a1 * pow(2 * x0, -1, P) % P)
    return None


def twist_point_outside_the_r_torsion(tag):
    """an on-curve point of the twist that is NOT in the r-torsion: hash x until x^3 + 3 / (9 + u) has a root (the cofactor is
    ~2^254, so a random curve point is outside the subgroup -- the class g2_decode's [r]Q loop exists for)"""
    bt = fields.f2_mul((3, 0), fields.f2_inv(fields.XI))
    k = 0
    while True:
        h = hashlib.sha256(b"%s/%d" % (tag, k)).digest()
        x = (int.from_bytes(h, "little") % P, int.from_bytes(hashlib.sha256(h).digest(), "little") % P)
        y = _fq2_sqrt(fields.f2_add(fields.f2_mul(fields.f2_sqr(x), x), bt))
        k += 1
        if y is None:
            continue
        q = (x, y)
        assert G2.is_on_curve(q)
        if G2.add(G2.mul(q, R - 1), q) is not None:      # [r]q, as (r - 1) q + q: the oracle's mul reduces its scalar mod r
            return q


def _flip(proof, pos, bit=0):
    t = bytearray(proof)
    t[pos] ^= 1 << bit
    return bytes(t)


def corruptions(proof, pub, other_pub, rnd, small):
    """(label, public inputs, proof) for every corruption class of the issue; `other_pub`: a neighbour's statement"""
    out = [("flip A", pub, _flip(proof, 5, 3)), ("flip B", pub, _flip(proof, 100, 1)), ("flip C", pub, _flip(proof, 200, 6))]
    for name, lo, hi in (("A", 0, 64), ("B", 64, 192), ("C", 192, 256)):
        out.append((name + " = infinity", pub, proof[:lo] + bytes(hi - lo) + proof[hi:]))
    for k in ((0, 3, 7) if small else range(8)):
        v = int.from_bytes(proof[32 * k:32 * k + 32], "little") + P
        if v < 1 << 256:
            out.append(("coordinate %d + p" % k, pub, proof[:32 * k] + _le(v) + proof[32 * k + 32:]))
    for _ in range(2 if small else 6):
        out.append(("random bytes below p", pub, b"".join(_le(rnd.randrange(P)) for _ in range(8))))
    out.append(("random bytes", pub, rnd.randbytes(256)))
    q = twist_point_outside_the_r_torsion(b"owshen verify batch")
    out.append(("B on the twist, outside the r-torsion", pub, proof[:64] + g2_to_bytes(q) + proof[192:]))
    out.append(("a neighbour's public inputs", other_pub, proof))
    out.append(("public input = r", [R] + pub[1:], proof))
    if pub[0] + R < 1 << 256:
        out.append(("public input + r", [pub[0] + R] + pub[1:], proof))
    out.append(("last public input = 2^256 - 1", pub[:-1] + [(1 << 256) - 1], proof))
    return out


def expected(blob, entries, threads=16):
    """og_verify's answer for every (pub, proof), through a thread pool (the host-only library)"""
    from owshen_amd import verify_only
    with ThreadPoolExecutor(threads) as ex:
        return np.array(list(ex.map(lambda e: bool(verify_only.verify(blob, e[0], e[1])), entries)), dtype=bool)


def run_batch(ctx, key, entries):
    pub = np.frombuffer(b"".join(_le(x) for e in entries for x in e[0]), dtype=np.uint8).reshape(len(entries), key.n_pub, 32)
    proofs = np.frombuffer(b"".join(e[1] for e in entries), dtype=np.uint8).reshape(len(entries), 256)
    return key.verify_batch(pub.copy(), proofs.copy())


def _oracle_says(inst_vk, pub, proof):
    return bool(og16.verify(inst_vk, pub, og16.proof_from_bytes(proof)))


def case_mixed_batch(ctx, small):
    """decision parity on a mixed batch, for a key with n_pub = 2 and one with n_pub = 6"""
    from owshen_amd import groth16 as g16
    rnd = random.Random(2024)
    seen = set()
    for n_pub, seed in ((2, 5), (6, 11)):
        inst = Instance(n_pub, seed)
        n_valid = 2 if small else 5
        valid = [inst.prove()] + [inst.prove([rnd.randrange(R) for _ in range(inst.n_in - 1)]) for _ in range(n_valid - 1)]
        entries, labels = [], []
        for k, (pub, proof) in enumerate(valid):
            entries.append((pub, proof)); labels.append("valid %d" % k)
        for k, (pub, proof) in enumerate(valid[:1] if small else valid[:2]):
            for label, cp, cpr in corruptions(proof, pub, valid[(k + 1) % len(valid)][0], rnd, small):
                entries.append((cp, cpr)); labels.append(label)
        want = expected(inst.blob, entries)
        with g16.VerifyingKey(ctx, inst.blob) as key:
            assert key.n_pub == n_pub and key.walk_steps == 102 and key.table_bytes == n_pub * 64 * 15 * 64
            got = run_batch(ctx, key, entries)
        assert got.tolist() == want.tolist(), [(l, bool(g), bool(w)) for l, g, w in zip(labels, got, want) if g != w]
        assert want[:len(valid)].all() and not want[len(valid):].any()      # accepts and rejects both occur, where they should
        for k in range(len(valid)):                                         # the oracle's verifier on a subset
            assert _oracle_says(inst.vk, *entries[k]) is True
        k = labels.index("a neighbour's public inputs")
        assert _oracle_says(inst.vk, *entries[k]) is False
        seen |= set(labels)

        # a valid proof under a key with an IC point at infinity: a statement whose second public input is 0 does not use IC_2
        pub0, proof0 = inst.prove([rnd.randrange(R), 0] + [rnd.randrange(R) for _ in range(inst.n_in - 3)])
        assert pub0[1] == 0
        vk_inf = dict(inst.vk, ic=list(inst.vk["ic"]))
        vk_inf["ic"][2] = None
        blob_inf = vk_blob(vk_inf)
        assert blob_inf[16 + 64 + 384 + 128:16 + 64 + 384 + 192] == bytes(64)
        e_inf = [(pub0, proof0), ([pub0[0], 5] + pub0[2:], proof0), ([pub0[0], R] + pub0[2:], proof0), (pub0, _flip(proof0, 9))]
        want = expected(blob_inf, e_inf)
        assert want.tolist() == [True, True, False, False]      # (x_2 is free when IC_2 is infinite, but it must still be < r)
        with g16.VerifyingKey(ctx, blob_inf) as key:
            assert run_batch(ctx, key, e_inf).tolist() == want.tolist()

        # vk_x at infinity: IC_0 := -(sum x_i IC_i) for this statement.  An honest proof does not verify under such a key (the
        # three remaining pairings do not cancel), but og_verify skips gamma's pairing there and so must the kernels: parity on
        # rejects here; case_vkx_infinity_accept builds, from the generators, a key and statement that is ACCEPTED that way.
        pub, proof = valid[0]
        acc = None
        for x, pt in zip(pub, inst.vk["ic"][1:]):
            acc = G1.add(acc, G1.mul(pt, x))
        vk_z = dict(inst.vk, ic=[G1.neg(acc)] + list(inst.vk["ic"][1:]))
        blob_z = vk_blob(vk_z)
        e_z = [(pub, proof), (valid[1][0], valid[1][1])]
        want = expected(blob_z, e_z)
        with g16.VerifyingKey(ctx, blob_z) as key:
            assert run_batch(ctx, key, e_z).tolist() == want.tolist() == [False, False]
    for must in ("flip A", "flip B", "flip C", "A = infinity", "B = infinity", "C = infinity", "coordinate 0 + p", "random bytes below p",
                 "B on the twist, outside the r-torsion", "a neighbour's public inputs", "public input = r", "public input + r"):
        assert must in seen, must


def case_vkx_infinity_accept(ctx):
    """a key and statement with vk_x = infinity that og_verify ACCEPTS, built directly from the generators: A = a G1, B = b G2,
    alpha = (a b + k) G1, beta = delta = G2, C = -k G1 and IC_0 = -x IC_1 (gamma is arbitrary: its pairing is skipped)"""
    from owshen_amd import groth16 as g16
    rnd = random.Random(77)
    a, b, k, x = (rnd.randrange(2, R) for _ in range(4))
    g1, g2 = G1.gen, G2.gen
    ic1 = G1.mul(g1, 12345)
    vk = {"alpha_g1": G1.mul(g1, (a * b + k) % R), "beta_g2": g2, "gamma_g2": G2.mul(g2, 3), "delta_g2": g2,
          "ic": [G1.neg(G1.mul(ic1, x)), ic1]}
    proof = g1_to_bytes(G1.mul(g1, a)) + g2_to_bytes(G2.mul(g2, b)) + g1_to_bytes(G1.neg(G1.mul(g1, k)))
    # e(-aG, bH) e((ab + k) G, H) e(-kG, H) = 1, and vk_x = -x IC_1 + x IC_1 = infinity
    blob = vk_blob(vk)
    entries = [([x], proof), ([(x + 1) % R], proof), ([x], _flip(proof, 3))]
    want = expected(blob, entries)
    assert want.tolist() == [True, False, False]
    with g16.VerifyingKey(ctx, blob) as key:
        assert run_batch(ctx, key, entries).tolist() == want.tolist()


def case_eip197_vector(ctx):
    """the published EIP-197 "jeff1" vector, embedded in the Groth16 predicate exactly as tests/test_external_pins.py does for
    og_verify (a key with n_pub = 0: A = -P1, B = Q1, alpha = P2, beta = Q2, IC_0 = G1, C = -G1, gamma = delta = G2)"""
    from owshen_amd import groth16 as g16
    from tests.test_external_pins import _jeff1, _vk_blob, G1_GEN, G2_GEN
    _w, p1, q1, p2, q2 = _jeff1()
    vk = _vk_blob(p2, q2, G2_GEN, G2_GEN, [G1_GEN])
    proof = g1_to_bytes(G1.neg(p1)) + g2_to_bytes(q1) + g1_to_bytes(G1.neg(G1_GEN))
    swapped = g1_to_bytes(G1.neg(p2)) + g2_to_bytes(q1) + g1_to_bytes(G1.neg(G1_GEN))
    t = bytearray(proof)
    t[3] ^= 0x10
    entries = [([], proof), ([], swapped), ([], bytes(t))]
    with g16.VerifyingKey(ctx, vk) as key:
        assert key.n_pub == 0 and key.table_bytes == 0
        assert run_batch(ctx, key, entries).tolist() == expected(vk, entries).tolist() == [True, False, False]
        assert key.verify_batch(np.zeros((0, 0, 32), dtype=np.uint8), np.zeros((0, 256), dtype=np.uint8)).tolist() == []   # n = 0
    with g16.VerifyingKey(ctx, _vk_blob(p1, q2, G2_GEN, G2_GEN, [G1_GEN])) as key:
        assert run_batch(ctx, key, entries[:1]).tolist() == [False]


def case_keys(ctx):
    """every malformed-key class of tests/test_verify_fuzz.py::test_verifying_key_bytes: where og_verify names the key invalid,
    og_vk_load answers OG_ERR_INVALID (-1); where og_verify only refuses the proof, the key loads and the batch refuses it too.
    Then two keys loaded at once, used alternately."""
    from owshen_amd import api, groth16 as g16, verify_only
    a, b = Instance(2, 5), Instance(6, 11)
    pub, proof = a.prove()
    blob = a.blob
    rnd = random.Random(2)
    variants = [blob[:cut] for cut in (0, 7, 8, 15, 16, 17, 80, len(blob) - 64, len(blob) - 1)]
    variants += [blob + b"\0", blob + blob[-64:], b"OWVK0002" + blob[8:]]
    variants += [blob[:8] + struct.pack("<Q", n) + blob[16:] for n in (0, 1, 3, 1 << 20, (1 << 64) - 1)]
    for pos in range(16, len(blob), 7):
        t = bytearray(blob)
        t[pos] ^= 1 << rnd.randrange(8)
        variants.append(bytes(t))
    variants += [blob[:16] + rnd.randbytes(len(blob) - 16) for _ in range(10)]
    n_invalid = n_loaded = 0
    for v in variants:
        try:
            want = verify_only.verify(v, pub, proof)
        except ValueError:
            want = "invalid"
        n_here = struct.unpack("<Q", v[8:16])[0] if len(v) >= 16 else None
        if want == "invalid" and n_here == 2 or n_here != 2:
            # (a header with another n_pub: og_verify's "count does not match" comes first there; og_vk_load has no count to
            # compare, so it judges the key by its own length rule -- none of these variants passes it)
            try:
                g16.VerifyingKey(ctx, v)
                raise AssertionError("a malformed key loaded: %d bytes" % len(v))
            except api.OwshenGpuError as e:
                assert e.code == -1, e
                assert "og_vk_load" in str(e)
            n_invalid += 1
        else:
            with g16.VerifyingKey(ctx, v) as key:
                assert run_batch(ctx, key, [(pub, proof)]).tolist() == [want]
            n_loaded += 1
    assert n_invalid >= 100, (n_invalid, n_loaded)      # (a flipped bit leaves a key point off its curve: none of these loads)
    # a well-formed key that is simply another key loads, and refuses the proof
    other = dict(a.vk, ic=[a.vk["ic"][0], a.vk["ic"][1], G1.mul(a.vk["ic"][2], 2)])
    with g16.VerifyingKey(ctx, vk_blob(other)) as key:
        assert run_batch(ctx, key, [(pub, proof)]).tolist() == [False] == expected(vk_blob(other), [(pub, proof)]).tolist()
    # two keys at once
    pub_b, proof_b = b.prove()
    ka, kb = g16.VerifyingKey(ctx, a.blob), g16.VerifyingKey(ctx, b.blob)
    for _ in range(2):
        assert run_batch(ctx, ka, [(pub, proof), (pub, _flip(proof, 70))]).tolist() == [True, False]
        assert run_batch(ctx, kb, [(pub_b, _flip(proof_b, 1)), (pub_b, proof_b)]).tolist() == [False, True]
    assert run_batch(ctx, ka, [(pub_b[:2], proof_b)]).tolist() == [False]      # the other key's proof
    ka.close(); kb.close()
    ka.close()                                                                 # closing twice is harmless


def case_final_exponentiation_pin(ctx):
    """The kernel's chain (easy part, then the x-power chain: og_verify's value raised to m = 2x(6x^2 + 3x + 1)) and og_verify's
    plain 2790-bit power agree on "is one", on Miller products of valid proofs (r-th-power residues: the plain power is 1) and of
    corrupted but well-formed ones (not residues).  Through the two seams of the hooks build (verify_gpu.hip, OG_AB_HOOKS)."""
    from owshen_amd import groth16 as g16
    lib = ctx._lib
    rnd = random.Random(8)
    inst = Instance(2, 5)
    valid = [inst.prove()] + [inst.prove([rnd.randrange(R) for _ in range(inst.n_in - 1)]) for _ in range(5)]
    entries = list(valid)
    for k in range(30):
        pub, proof = valid[k % len(valid)]
        kind = k % 3
        if kind == 0:
            entries.append(([rnd.randrange(R), pub[1]], proof))                                  # another statement
        elif kind == 1:
            a2 = G1.mul(og16.proof_from_bytes(proof)[0], 2 + k)
            entries.append((pub, g1_to_bytes(a2) + proof[64:]))                                  # another A (on the curve)
        else:
            entries.append((pub, proof[:192] + g1_to_bytes(G1.mul(G1.gen, 1000 + k))))           # another C (on the curve)
    n = len(entries)
    pub = np.frombuffer(b"".join(_le(x) for e in entries for x in e[0]), dtype=np.uint8).reshape(n, 2, 32).copy()
    proofs = np.frombuffer(b"".join(e[1] for e in entries), dtype=np.uint8).reshape(n, 256).copy()
    with g16.VerifyingKey(ctx, inst.blob) as key:
        pub_d, proofs_d = ctx.to_device(pub), ctx.to_device(proofs)
        f = np.zeros((n, 108), dtype=np.uint32)
        state = np.zeros(n, dtype=np.uint32)
        ctx._pre()
        fn = lib.og_hook_verify_miller_d
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        ctx._check(fn(ctx._h, key._h, ctx.ptr(pub_d), ctx.ptr(proofs_d), n, f.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p)))
        assert (state & 1).all()                                     # all well-formed: every entry reached the Miller loop
        chain, plain = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        fe = lib.og_hook_final_exp_d
        fe.restype = C.c_int
        fe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        ctx._check(fe(ctx._h, key._h, f.ctypes.data_as(C.c_void_p), n, chain.ctypes.data_as(C.c_void_p), plain.ctypes.data_as(C.c_void_p)))
    assert chain.tolist() == plain.tolist()
    assert plain[:len(valid)].tolist() == [1] * len(valid) and not plain[len(valid):].any()
    assert plain.tolist() == expected(inst.blob, entries).astype(np.uint32).tolist()


def chain_multiplier():
    """the x-power chain of k_vfy_finalexp replayed on exponents (an element of the cyclotomic subgroup is tracked as its exponent
    modulo Phi_12(p); conjugation = negation, Frobenius = multiplication by p): returns m with chain = m * (p^4 - p^2 + 1) / r"""
    x = fields.BN_X
    phi = P ** 4 - P ** 2 + 1
    assert phi % R == 0
    h = phi // R
    nx = lambda e: -x * e % phi
    fr = lambda e, k: e * pow(P, k, phi) % phi
    r0 = 1
    y0 = nx(r0); y1 = 2 * y0; y2 = 2 * y1; y3 = y2 + y1; y4 = nx(y3); y5 = 2 * y4; y6 = nx(y5)
    y3, y6 = -y3, -y6
    y7 = y6 + y4; y8 = y7 + y3; y9 = y8 + y1; y10 = y8 + y4; y11 = y10 + r0
    y13 = fr(y9, 1) + y11
    y14 = fr(y8, 2) + y13
    y16 = (fr(-r0 + y9, 3) + y14) % phi
    assert y16 % h == 0
    return y16 // h
