"""og_ptau_verify / og_pk_verify cases shared by the CPU-interpreter run (test_emu_ptau_verify.py) and the GPU run
(test_gpu_ptau_verify.py).  Files come from a known (tau, alpha, beta) through the writer of tests/ptau_cases.py; substitute
points are made by the library's fixed-base multiplication, so every one of them is on its curve and in the subgroup and only the
pairing checks can tell.  Every case asserts the exact mask: bit k of og_ptau_verify is PTAU_CHECKS[k], of og_pk_verify
KEY_CHECKS[k] (owshen_amd/ptau.py).  The sizes: power 1 (tauG1 has 3 points, every other section one pair), 2 (the smallest with
an interior tauG1 point that is not the ratio point), 5 (63 / 32 points: inside one wave), 7 (255 / 128: past one workgroup of the
scalar kernel and one block of the sort), 10 with the deposit key."""
import random
import struct

import numpy as np
import pytest

from oracle.py import fields
from tests import ptau_cases as pc
from tests.r1cs_util import random_r1cs

R, P = fields.R, fields.P
TAU_G1, TAU_G2, ALPHA_G1, BETA_G1, BETA_G2 = 1, 2, 4, 8, 16          # og_ptau_verify
HEADER, QUERIES, IC, DELTA, L, H = 1, 2, 4, 8, 16, 32                 # og_pk_verify


def _canon(ctx, group, scalars):
    """[k] G as canonical bytes, one after the other"""
    from owshen_amd import api, groth16 as g16
    base = g16.G1_GEN_BYTES if group == 1 else g16.G2_GEN_BYTES
    return np.asarray(ctx.to_host(ctx.scalar_mul(group, base, ctx.to_device(api.ints_to_bytes(scalars))))).tobytes()


def _patched(sections, sid, index, point):
    """the file with point `index` of section `sid` replaced (file encoding)"""
    out = []
    for s, body in sections:
        if s == sid:
            body = body[:index * len(point)] + point + body[(index + 1) * len(point):]
        out.append((s, body))
    return pc._file(out)


# ---- og_ptau_verify -----------------------------------------------------------------------------------------------------------
def case_valid_file(ctx, power):
    from owshen_amd import ptau
    data = pc.make_ptau(ctx, power, *pc._toxic(40 + power))
    assert ptau.verify_mask(ctx, data) == 0


def tampered_files(ctx, power):
    """name -> (a function that makes the file, the exact mask).  The replaced points are multiples of the generators that
    nobody's tau produces."""
    tau, alpha, beta = toxic = pc._toxic(40 + power)
    sec = pc.ptau_sections(ctx, power, *toxic)
    n = 1 << power
    rnd = random.Random(900 + power)
    k1, k2, t2, b2, x = (rnd.randrange(2, R) for _ in range(5))
    g1 = lambda k: pc._points(ctx, 1, [k])                                                 # noqa: E731
    g2 = lambda k: pc._points(ctx, 2, [k])                                                 # noqa: E731

    def forged():
        # tauG1[2] += x G1 and tauG1[2n - 2] += (tau - 1) x G1: the sum over points 0 .. 2n - 3 grows by x G1, the sum over points
        # 1 .. 2n - 2 by x G1 + (tau - 1) x G1 = tau x G1 -- with all challenge scalars EQUAL the two sums still match
        new = pc._points(ctx, 1, [(pow(tau, 2, R) + x) % R, (pow(tau, 2 * n - 2, R) + (tau - 1) * x) % R])
        body = dict(sec)[2]
        return pc._file(pc._replace(sec, 2, body[:128] + new[:64] + body[192:-64] + new[64:]))
    out = {
        "tauG1[1], also the ratio of the tauG2 check": (lambda: _patched(sec, 2, 1, g1(k1)), TAU_G1 | TAU_G2),
        "tauG1[2n - 2], the last point, which only the shifted sum holds": (lambda: _patched(sec, 2, 2 * n - 2, g1(k1)), TAU_G1),
        "tauG2[1], the ratio of three other checks": (lambda: _patched(sec, 3, 1, g2(t2)), TAU_G1 | TAU_G2 | ALPHA_G1 | BETA_G1),
        "alphaTauG1[0]": (lambda: _patched(sec, 4, 0, g1(k1)), ALPHA_G1),
        "alphaTauG1 built consistently from another tau": (lambda: pc._file(pc._replace(sec, 4, dict(pc.ptau_sections(ctx, power, t2, alpha, beta))[4])), ALPHA_G1),
        "betaTauG1's last point": (lambda: _patched(sec, 5, n - 1, g1(k2)), BETA_G1),
        "betaG2": (lambda: _patched(sec, 6, 0, g2(b2)), BETA_G2),
        "infinity in betaTauG1": (lambda: _patched(sec, 5, n - 1, bytes(64)), BETA_G1),
    }
    if power >= 2:
        out["tauG1[2]"] = (lambda: _patched(sec, 2, 2, g1(k1)), TAU_G1)
        out["tauG2[n - 1]"] = (lambda: _patched(sec, 3, n - 1, g2(k2)), TAU_G2)
        out["a forgery an unweighted sum accepts"] = (forged, TAU_G1)
    return out


ALL_TAMPERED = ("tauG1[1], also the ratio of the tauG2 check", "tauG1[2n - 2], the last point, which only the shifted sum holds",
                "tauG2[1], the ratio of three other checks", "alphaTauG1[0]", "alphaTauG1 built consistently from another tau",
                "betaTauG1's last point", "betaG2", "infinity in betaTauG1", "tauG1[2]", "tauG2[n - 1]", "a forgery an unweighted sum accepts")
# what a larger size can still get wrong: the ends of the sums, and the weights
SIZE_TAMPERED = ("tauG1[2n - 2], the last point, which only the shifted sum holds", "tauG2[n - 1]", "betaTauG1's last point", "tauG1[2]",
                 "a forgery an unweighted sum accepts")


def case_tampered_files(ctx, power, names):
    from owshen_amd import ptau
    made = tampered_files(ctx, power)
    got, want = {}, {}
    for name in names:
        if name in made:                                    # (power 1 has no interior point)
            got[name], want[name] = ptau.verify_mask(ctx, made[name][0]()), made[name][1]
    assert got == want and len(got) >= 4
    if "betaG2" in got:
        assert ptau.verify(ctx, made["betaG2"][0]()) == ["betaG2"]
        assert b"og_ptau_verify" in ctx._lib.og_last_error() and b"betaG2" in ctx._lib.og_last_error()


def case_file_refusals(ctx):
    """the whole of every section is decoded: a point off the curve past what a key of the 25-constraint circuit reads"""
    import ctypes as C
    from owshen_amd import ptau
    from owshen_amd.api import OwshenGpuError
    r1cs = pc._small(25, 3)
    sec = pc.ptau_sections(ctx, 6, *pc._toxic(66))
    body = bytearray(dict(sec)[4])
    body[64 * 40 + 32:64 * 40 + 64] = (12345).to_bytes(32, "little")
    data = pc._file(pc._replace(sec, 4, bytes(body)))
    ptau.setup(ctx, r1cs, data)                                        # entry 40 of a domain of 32: not looked at
    with pytest.raises(OwshenGpuError) as e:
        ptau.verify_mask(ctx, data)
    assert e.value.code == -1 and "og_ptau_verify" in str(e.value) and "section 4" in str(e.value) and "curve" in str(e.value)
    with pytest.raises(OwshenGpuError) as e:
        ptau.verify_mask(ctx, pc._file([s for s in sec if s[0] != 5]))
    assert "section 5" in str(e.value)
    x, y = pc.twist_point_outside_the_subgroup()
    rogue = pc._enc(b"".join(v.to_bytes(32, "little") for v in (x[0], x[1], y[0], y[1])))
    with pytest.raises(OwshenGpuError) as e:
        ptau.verify_mask(ctx, _patched(sec, 3, 40, rogue))
    assert "section 3" in str(e.value) and "subgroup" in str(e.value)
    good = pc._file(sec)
    buf = (C.c_uint8 * len(good)).from_buffer_copy(good)
    assert ctx._lib.og_ptau_verify(ctx._h, buf, len(good), None) == -1 and b"og_ptau_verify: null" in ctx._lib.og_last_error()


def case_null_handles(lib):
    """refused before any device is touched (runs on a host without one)"""
    import ctypes as C
    buf = (C.c_uint8 * 64)()
    mask = C.c_uint32(7)
    assert lib.og_ptau_verify(None, buf, 64, C.byref(mask)) == -1 and b"og_ptau_verify: null" in lib.og_last_error()
    assert lib.og_pk_verify(None, None, buf, 64, buf, 64, buf, 64, C.byref(mask)) == -1 and b"og_pk_verify: null" in lib.og_last_error()


def case_refused_while_a_job_is_pending(ctx):
    """both calls use the lone MSM's scratch, which is a submitted prove call's scratch too: refused until the job is waited for"""
    from owshen_amd import circuit, ptau
    from owshen_amd.api import OwshenGpuError
    from tests import withdraw_cases as wc
    r1cs = pc._small(25, 3)
    data = pc.make_ptau(ctx, r1cs.log_d, *pc._toxic(125))
    key = ptau.setup(ctx, r1cs, data)
    rnd = random.Random(11)
    _r1, _blob, _vk, wpk, _close = wc._key(ctx, 1, 2, 3)
    packed = ctx.to_device(np.stack([wc._pack(circuit, wc._inputs(rnd, 1))]))
    job = circuit.submit_from_inputs(ctx, wpk, 1, packed, [(rnd.randrange(R), rnd.randrange(R))], 2, 3)
    try:
        for call in (lambda: ptau.verify_mask(ctx, data), lambda: ptau.verify_key_mask(ctx, r1cs, data, *key)):
            with pytest.raises(OwshenGpuError) as e:
                call()
            assert e.value.code == -1 and "og_job_wait" in str(e.value)
    finally:
        job.wait()
    assert ptau.verify_mask(ctx, data) == 0 and ptau.verify_key_mask(ctx, r1cs, data, *key) == 0


# ---- og_pk_verify -------------------------------------------------------------------------------------------------------------
class Layout:
    """where the parts of an OWPK0001 blob lie, from the blob's own header (the layout owshen_amd/groth16.py serialises)"""

    def __init__(self, pk):
        from owshen_amd import groth16 as g16
        assert pk[:8] == g16.PK_MAGIC
        _magic, self.m, self.l, power, n_rows, nnz_a, nnz_b, nnz_c, self.flag, _zero = struct.unpack("<10Q", pk[:80])
        pad = lambda n: len(g16._pad32(bytes(n)))                                          # noqa: E731
        self.delta1, self.delta2 = 80 + 128, 80 + 384
        off = 80 + 512
        for nnz in (nnz_a, nnz_b, nnz_c):
            off += pad(4 * (n_rows + 1)) + pad(4 * nnz) + pad(32 * nnz)
        self.a = off
        self.l_off = off + 2 * pad(64 * self.m) + pad(128 * self.m)
        self.nl, self.nh = self.m - self.l - 1, (1 << power) - 1
        self.h_off = self.l_off + pad(64 * self.nl)
        assert self.h_off + pad(64 * self.nh) == len(pk)
        self.vk_delta2 = 16 + 64 + 256


def _put(blob, off, new):
    return blob[:off] + new + blob[off + len(new):]


def _swapped(blob, off, i, j):
    a, b = blob[off + 64 * i:off + 64 * i + 64], blob[off + 64 * j:off + 64 * j + 64]
    assert a != b and a != bytes(64) and b != bytes(64)
    return _put(_put(blob, off + 64 * i, b), off + 64 * j, a)


def case_valid_keys(ctx, r1cs, seed, extra_power=0):
    """og_setup_ptau's key, one and two contributions on it, og_setup with gamma = 1 and a delta of its own: all the file's keys"""
    from owshen_amd import groth16 as g16, ptau
    toxic = pc._toxic(seed)
    data = pc.make_ptau(ctx, r1cs.log_d + extra_power, *toxic)
    rnd = random.Random(seed + 7)
    d1, d2, d3 = (rnd.randrange(2, R) for _ in range(3))
    pk0, vk0 = ptau.setup(ctx, r1cs, data)
    one = ptau.contribute(ctx, pk0, vk0, d1)
    two = ptau.contribute(ctx, *one, d2)
    pk3, vk3 = g16.setup(ctx, r1cs, *toxic, 1, d3)
    got = {"delta = 1": ptau.verify_key_mask(ctx, r1cs, data, pk0, vk0), "one contribution": ptau.verify_key_mask(ctx, r1cs, data, *one),
           "two contributions": ptau.verify_key_mask(ctx, r1cs, data, *two),
           "og_setup's": ptau.verify_key_mask(ctx, r1cs, data, pk3, g16.vk_to_bytes(vk3))}
    assert got == dict.fromkeys(got, 0)


def _other_coefficient(r1cs):
    """the same circuit shape with ONE coefficient of A changed, on a private wire: another circuit whose key has the same header"""
    from owshen_amd import groth16 as g16
    nc = r1cs.n_constraints

    def rows(mat, val=None):                                # the constraint rows, without the input-consistency rows R1CS appends
        nnz = int(mat.ptr[nc])
        return g16.SparseMatrix(mat.ptr[:nc + 1], mat.col[:nnz], (mat.val if val is None else val)[:nnz], mat.n_cols)
    e = next(i for i, c in enumerate(r1cs.a.col[:int(r1cs.a.ptr[nc])]) if c > r1cs.n_pub)
    val = r1cs.a.val.copy()
    val[e] = np.frombuffer((int.from_bytes(bytes(val[e]), "little") + 5).to_bytes(32, "little"), np.uint8)
    return g16.R1CS(r1cs.n_wires, r1cs.n_pub, rows(r1cs.a, val), rows(r1cs.b), rows(r1cs.c))


def case_foreign_keys(ctx):
    """keys that are somebody's, but not this circuit's from this file"""
    from owshen_amd import groth16 as g16, ptau, zkey as zk
    from owshen_amd.api import OwshenGpuError
    r1cs = pc._small(25, 3)
    tau, alpha, beta = toxic = pc._toxic(77)
    data = pc.make_ptau(ctx, r1cs.log_d, *toxic)
    rnd = random.Random(78)
    gamma, delta, alpha2 = (rnd.randrange(2, R) for _ in range(3))
    got, want = {}, {}

    def check(name, mask, r, pk, vk):
        got[name], want[name] = ptau.verify_key_mask(ctx, r, data, pk, vk), mask
    pk, vk = g16.setup(ctx, r1cs, tau, alpha, beta, gamma, delta)
    check("gamma != 1", HEADER | IC, r1cs, pk, g16.vk_to_bytes(vk))
    # one coefficient of A on a private wire: the matrices, the A query and that wire's L entry (beta A_i + ..) differ; H knows no circuit
    other = _other_coefficient(r1cs)
    check("another circuit of the same shape", HEADER | QUERIES | L, r1cs, *ptau.setup(ctx, other, data))
    check("a circuit of another shape", 63, r1cs, *ptau.setup(ctx, pc._small(24, 3), data))
    # alpha enters alpha1 and, through alpha B_i, the IC / L entries of the wires that occur in B
    b_cols = set(int(c) for c in r1cs.b.col)
    mask = HEADER | (IC if any(c <= r1cs.n_pub for c in b_cols) else 0) | (L if any(c > r1cs.n_pub for c in b_cols) else 0)
    check("a file with another alpha", mask, r1cs, *ptau.setup(ctx, r1cs, pc.make_ptau(ctx, r1cs.log_d, tau, alpha2, beta)))
    assert got == want
    assert want["a file with another alpha"] & L                        # (the 25-constraint circuit does have private wires in B)
    n_wires, cons, _z0 = random_r1cs(25, 3, seed=25 + 5000)
    from oracle.py import zkey as zo
    flag1 = zk.import_zkey(ctx, zo.write_zkey(zo.snarkjs_setup(n_wires, 3, cons, tau, alpha, beta, 1, delta)))
    assert Layout(flag1[0]).flag == 1
    with pytest.raises(OwshenGpuError) as e:
        ptau.verify_key_mask(ctx, r1cs, data, *flag1)
    assert e.value.code == -1 and "og_pk_verify" in str(e.value) and ".r1cs" in str(e.value)


def tampered_keys(ctx, data, delta1_key, contributed):
    """name -> ((pk, vk), the exact mask), from a valid pair with delta = 1 and a valid contributed pair"""
    pk0, _vk0 = delta1_key
    pk, vk = contributed
    lay = Layout(pk)
    rnd = random.Random(4242)
    g1 = _canon(ctx, 1, [rnd.randrange(2, R) for _ in range(5)])
    g2 = _canon(ctx, 2, [rnd.randrange(2, R)])
    off_curve = _put(pk, lay.l_off + 64 * (lay.nl // 2) + 32, ((int.from_bytes(pk[lay.l_off + 64 * (lay.nl // 2) + 32:][:32], "little") + 1) % P).to_bytes(32, "little"))
    return {
        "delta1 replaced": ((_put(pk, lay.delta1, g1[:64]), vk), DELTA),
        "the verifying key's delta2 is another": ((pk, _put(vk, lay.vk_delta2, g2)), DELTA),
        "the H query from before the contribution": ((_put(pk, lay.h_off, pk0[lay.h_off:lay.h_off + 64 * lay.nh]), vk), H),
        "the L query from before the contribution": ((_put(pk, lay.l_off, pk0[lay.l_off:lay.l_off + 64 * lay.nl]), vk), L),
        "first L entry": ((_put(pk, lay.l_off, g1[64:128]), vk), L),
        "last L entry": ((_put(pk, lay.l_off + 64 * (lay.nl - 1), g1[128:192]), vk), L),
        "first H entry": ((_put(pk, lay.h_off, g1[192:256]), vk), H),
        "last H entry": ((_put(pk, lay.h_off + 64 * (lay.nh - 1), g1[256:320]), vk), H),
        "two L entries swapped: the plain sum is unchanged": ((_swapped(pk, lay.l_off, 1, lay.nl - 2), vk), L),
        "two H entries swapped": ((_swapped(pk, lay.h_off, 0, lay.nh - 1), vk), H),
        "an L entry off the curve": ((off_curve, vk), L),
        "delta2 is infinity, in both keys": ((_put(pk, lay.delta2, bytes(128)), _put(vk, lay.vk_delta2, bytes(128))), DELTA | L | H),
    }


def case_tampered_keys(ctx, part):
    """the tampered keys of the 25-constraint circuit, in three parts of four (each call rebuilds the delta = 1 key)"""
    from owshen_amd import ptau
    r1cs = pc._small(25, 3)
    data = pc.make_ptau(ctx, r1cs.log_d, *pc._toxic(125))
    delta1_key = ptau.setup(ctx, r1cs, data)
    contributed = ptau.contribute(ctx, *delta1_key, random.Random(126).randrange(2, R))
    made = tampered_keys(ctx, data, delta1_key, contributed)
    assert len(made) == 12
    got, want = {}, {}
    for name in list(made)[4 * part:4 * part + 4]:
        pair, mask = made[name]
        got[name], want[name] = ptau.verify_key_mask(ctx, r1cs, data, *pair), mask
    assert got == want and len(got) == 4
    if "first H entry" in got:
        assert ptau.verify_key(ctx, r1cs, data, *made["first H entry"][0]) == ["H"] and b"og_pk_verify" in ctx._lib.og_last_error()


def case_exported_and_imported_key(ctx):
    """a contributed key that went out through og_zkey_export and came back through og_zkey_import beside its r1cs"""
    from owshen_amd import ptau, zkey as zk
    r1cs = pc._small(25, 3)
    data = pc.make_ptau(ctx, r1cs.log_d, *pc._toxic(555))
    pk, vk = ptau.contribute(ctx, *ptau.setup(ctx, r1cs, data), 0xabcdef123)
    back = zk.import_zkey(ctx, zk.export_zkey(ctx, pk, vk), zk.write_r1cs(r1cs, lib=ctx._lib))
    assert ptau.verify_key_mask(ctx, r1cs, data, *back) == 0


def case_deposit_key(ctx):
    """power 10: the deposit circuit's file (the one tests/ptau_cases.py builds, once per process) and its contributed key"""
    from owshen_amd import ptau
    r1cs = pc._deposit(ctx)
    data = pc.make_ptau(ctx, 10, *pc._toxic(735))
    assert ptau.verify_mask(ctx, data) == 0
    pk, vk = ptau.contribute(ctx, *ptau.setup(ctx, r1cs, data), random.Random(4).randrange(2, R))
    lay = Layout(pk)
    got = {"valid": ptau.verify_key_mask(ctx, r1cs, data, pk, vk),
           "H swapped": ptau.verify_key_mask(ctx, r1cs, data, _swapped(pk, lay.h_off, 5, lay.nh - 3), vk),
           "L swapped": ptau.verify_key_mask(ctx, r1cs, data, _swapped(pk, lay.l_off, 3, lay.nl - 1), vk)}
    assert got == {"valid": 0, "H swapped": H, "L swapped": L}


# ---- the command line ---------------------------------------------------------------------------------------------------------
def case_cli(ctx, tmp_path, capsys):
    from owshen_amd import ptau, zkey as zk
    r1cs = pc._small(25, 3)
    sec = pc.ptau_sections(ctx, r1cs.log_d, *pc._toxic(555))
    data = pc._file(sec)
    pk, vk = ptau.contribute(ctx, *ptau.setup(ctx, r1cs, data), 0xabcdef123)
    lay = Layout(pk)
    files = {"c.r1cs": zk.write_r1cs(r1cs, lib=ctx._lib), "pot.ptau": data, "key.zkey": zk.export_zkey(ctx, pk, vk),
             "bad.zkey": zk.export_zkey(ctx, _swapped(pk, lay.l_off, 1, lay.nl - 2), vk),
             "bad.ptau": _patched(sec, 2, 2, pc._points(ctx, 1, [987654321]))}
    path = {}
    for name, body in files.items():
        path[name] = str(tmp_path / name)
        with open(path[name], "wb") as f:
            f.write(body)
    capsys.readouterr()
    assert zk.main(["verify", path["c.r1cs"], path["pot.ptau"], path["key.zkey"]], ctx=ctx) == 0
    assert zk.main(["ptau-verify", path["pot.ptau"]], ctx=ctx) == 0
    assert "FAILED" not in capsys.readouterr().out
    assert zk.main(["verify", path["c.r1cs"], path["pot.ptau"], path["bad.zkey"]], ctx=ctx) == 1
    assert capsys.readouterr().out.strip() == "FAILED: L"
    assert zk.main(["ptau-verify", path["bad.ptau"]], ctx=ctx) == 1
    assert capsys.readouterr().out.strip() == "FAILED: tauG1"
