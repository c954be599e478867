// snarkjs key and witness files at the boundary: `.zkey` -> this library's OWPK0001 / OWVK0001 blobs (og_zkey_import),
// the way back (og_zkey_export), `.wtns` <-> canonical witness bytes (og_wtns_read / og_wtns_write).
//
// No reference counterpart: the snapshot holds no prover and no key; the lineage BASELINE.json's north_star
// names proved with circom / snarkjs, and VERDICT r5 asks for "an import path for keys this repository did not make".  The
// container and the Groth16 sections are restated in oracle/py/zkey.py (the oracle of this file and the tests' writer), with
// the upstream function each fact comes from; nothing here has met a file snarkjs itself wrote -- there is none in this
// environment -- so the importer checks what it CAN check on any file: both primes, every section
// length against the header, every coordinate < q, every point on its curve (a mis-read encoding leaves the curve), every
// coefficient < r and inside the matrix; and a proof made with an imported key is judged by og_verify against the imported
// verifying key.
//
// What an import has to bridge (oracle/py/zkey.py has the derivations):
//   * points: affine, little-endian MONTGOMERY numbers with R = 2^256            -> canonical (k_lem_import; R here is 2^261)
//   * coefficients: value x R^2 mod r as plain integers, matrices A and B only     -> canonical CSR; the prover takes
//     C z = (A z) o (B z) for such a key (OWPK header flag 1; groth16.hip k_mul_rows)
//   * constraint c sits at w^c with ffjavascript's root w = 5^((r-1)/d); this library's row i at 7^((r-1)/d)^i (ntt.hip,
//     the reference's `Fp` generator, /root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:9): the same points
//     in another order                                                               -> a permutation of the rows
//   * the H section holds L_{2i+1}(tau) / delta . G1 over the size-2d domain (the ODD points), this library's H query
//     tau^j Z(tau) / delta . G1: since x^j Z(x) vanishes on the domain and equals -2 psi^j w^(i j) at psi^(2i+1),
//         H[j] = -2 psi^j  sum_i w^(i j) H'[i]
//     -- a DFT over group elements, run here as a radix-2 decimation-in-frequency FFT whose butterflies multiply a POINT
//     by a twiddle (k_ecntt_stage: (d / 2) log d scalar multiplications, ~45 ms for d = 2^17).  The prover itself is untouched:
//     an imported key proves through exactly the kernels every other key does, and the proof is the one snarkjs' own
//     algorithm gives for the same (r, s) (tests: oracle/py/zkey.snarkjs_prove, byte for byte).
#include "ctx.h"
#include "msm.hip.h"
#include "field.hip.h"
#include "ec.hip.h"
#include "snarkfile.hip.h"  // the container, the point decode kernel, the DFT over points: shared with ptau.hip
#include "key_blob.h"
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <memory>
#include <vector>

namespace og {

struct ZHeader {
  uint64_t m = 0, l = 0, d = 0;
  int power = 0;
};

// the domain's roots as ffjavascript numbers them, and the row <-> constraint permutation
struct ZDomain {
  Fr w, psi;     // primitive d-th and 2d-th roots (ffjavascript's), Montgomery
  uint64_t k;    // this library's row i <-> constraint i k mod d
};
static int zdomain(int power, const std::string& who, ZDomain* out) {
  const FfRoots& f = ff_roots();
  OG_REQUIRE(f.ok, who + ": internal: 5 is not the smallest quadratic non-residue of the scalar field");
  OG_REQUIRE(power >= 1 && power <= 27, who + ": domain must hold 2 .. 2^27 points");
  out->w = zfr_pow2k(f.w28_ff, 28 - power);
  out->psi = zfr_pow2k(f.w28_ff, 27 - power);
  out->k = zfr_dlog_pow2(out->w, zfr_pow2k(f.w28_own, 28 - power), power);
  return OG_OK;
}

// (row, signal, value) entries of one matrix -> CSR over d rows: columns ascending, duplicates summed, zeros dropped, values canonical
struct ZEnt {
  uint32_t row, sig;
  Fr v;  // Montgomery
};
static void zcsr(std::vector<ZEnt>& ent, uint64_t d, std::vector<uint32_t>& ptr, std::vector<uint32_t>& col, std::vector<uint8_t>& val) {
  std::stable_sort(ent.begin(), ent.end(), [](const ZEnt& a, const ZEnt& b) { return a.row != b.row ? a.row < b.row : a.sig < b.sig; });
  ptr.assign(d + 1, 0);
  col.clear();
  val.clear();
  for (size_t i = 0; i < ent.size();) {
    size_t j = i;
    Fr acc = Fr::zero();
    for (; j < ent.size() && ent[j].row == ent[i].row && ent[j].sig == ent[i].sig; j++) acc = fe_add(acc, ent[j].v);
    if (!acc.is_zero()) {
      col.push_back(ent[i].sig);
      val.resize(val.size() + 32);
      zfr_store(&val[val.size() - 32], fe_from_mont(acc));
      ptr[ent[i].row + 1]++;
    }
    i = j;
  }
  for (uint64_t r = 0; r < d; r++) ptr[r + 1] += ptr[r];
}

// r1cs (optional): the circuit the key was made for (og_r1cs_read of circom's .r1cs).  Its A and B matrices must be the key's
// coefficient section, row for row; its C matrix then rides in the imported key (header flag 0), and the prover refuses a
// witness that violates a constraint exactly as it does for a key of og_setup.
static int zkey_import(og_ctx* ctx, const uint8_t* data, size_t len, const og_r1cs* r1cs, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk) {
  const std::string who = "og_zkey_import";
  BinFile bf;
  OG_TRY(binfile_parse(data, len, "zkey", 1, who, &bf));
  for (uint32_t id = 1; id <= 9; id++) OG_REQUIRE(bf.sec.count(id), who + ": section " + std::to_string(id) + " missing");
  OG_REQUIRE(bf.sec[1].second >= 4 && rd32(bf.sec[1].first) == 1, who + ": not a Groth16 key (protocol id != 1)");
  const uint8_t* h = bf.sec[2].first;
  OG_REQUIRE(bf.sec[2].second == 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128, who + ": header section has the wrong length for BN254");
  OG_REQUIRE(rd32(h) == 32 && memcmp(h + 4, FQ_BYTES, 32) == 0, who + ": the base field is not BN254's");
  OG_REQUIRE(rd32(h + 36) == 32 && memcmp(h + 40, FR_BYTES, 32) == 0, who + ": the scalar field is not BN254's");
  ZHeader z;
  z.m = rd32(h + 72); z.l = rd32(h + 76); z.d = rd32(h + 80);
  OG_REQUIRE(z.d >= 2 && (z.d & (z.d - 1)) == 0, who + ": domain size is not a power of two >= 2");
  while (((uint64_t)1 << z.power) < z.d) z.power++;
  OG_REQUIRE(z.m >= 1 && z.l < z.m && z.m < (1ull << 31), who + ": bad wire counts");
  const uint64_t m = z.m, l = z.l, d = z.d, nl = m - l - 1;
  const uint64_t want[10] = {0, 0, 0, (l + 1) * 64, 0, m * 64, m * 64, m * 128, nl * 64, d * 64};
  for (uint32_t id : {3u, 5u, 6u, 7u, 8u, 9u})
    OG_REQUIRE(bf.sec[id].second == want[id], who + ": section " + std::to_string(id) + " has " + std::to_string(bf.sec[id].second) +
                                                  " bytes, the header asks for " + std::to_string(want[id]));
  ZDomain dom;
  OG_TRY(zdomain(z.power, who, &dom));
  // ---- coefficients -> CSR rows (A, B), canonical
  const uint8_t* cs = bf.sec[4].first;
  OG_REQUIRE(bf.sec[4].second >= 4, who + ": coefficient section truncated");
  const uint64_t n_coef = rd32(cs);
  OG_REQUIRE(bf.sec[4].second == 4 + n_coef * 44, who + ": coefficient section length does not match its count");
  Fr ri2 = Fr::one();  // 2^-512 mod r, Montgomery
  for (int i = 0; i < 512; i++) ri2 = fe_dbl(ri2);
  ri2 = fe_inv(ri2);
  const uint64_t kinv = inv_mod_pow2(dom.k, z.power);
  std::vector<ZEnt> ent[2];
  for (uint64_t i = 0; i < n_coef; i++) {
    const uint8_t* e = cs + 4 + i * 44;
    const uint32_t mt = rd32(e), c = rd32(e + 4), sg = rd32(e + 8);
    const Fr raw = zfr_load(e + 12);
    OG_REQUIRE(mt <= 1 && c < d && sg < m && fe_lt_modulus(raw), who + ": coefficient " + std::to_string(i) + " out of range");
    ent[mt].push_back({(uint32_t)((c * kinv) & (d - 1)), sg, fe_mul(fe_to_mont(raw), ri2)});
  }
  QapRows rows;  // over all d rows of the domain
  for (int k = 0; k < 2; k++) zcsr(ent[k], d, rows.ptr[k], rows.col[k], rows.val[k]);
  rows.ptr[2].assign(d + 1, 0);
  uint64_t flags = 1;  // no .r1cs given: C z = (A z) o (B z)
  if (r1cs) {
    const uint64_t nc = r1cs->n_constraints;
    OG_REQUIRE(r1cs->n_wires == m && r1cs->n_pub == l, who + ": the .r1cs has " + std::to_string(r1cs->n_wires) + " wires / " + std::to_string(r1cs->n_pub) +
                                                           " public, the .zkey " + std::to_string(m) + " / " + std::to_string(l));
    OG_REQUIRE(nc + l + 1 <= d, who + ": the .r1cs has more constraints than the key's domain holds");
    std::vector<ZEnt> re[3];
    for (int k = 0; k < 3; k++) {
      OG_REQUIRE(r1cs->ptr[k].size() == nc + 1 && r1cs->val[k].size() == r1cs->col[k].size() * 32, who + ": malformed R1CS");
      for (uint64_t c = 0; c < nc; c++)
        for (uint32_t e = r1cs->ptr[k][c]; e < r1cs->ptr[k][c + 1]; e++) {
          const Fr v = zfr_load(&r1cs->val[k][(size_t)e * 32]);
          OG_REQUIRE(r1cs->col[k][e] < m && fe_lt_modulus(v), who + ": R1CS entry out of range");
          re[k].push_back({(uint32_t)((c * kinv) & (d - 1)), r1cs->col[k][e], fe_to_mont(v)});
        }
    }
    for (uint64_t s = 0; s <= l; s++) re[0].push_back({(uint32_t)(((nc + s) * kinv) & (d - 1)), (uint32_t)s, Fr::one()});  // the public-input rows
    std::vector<uint32_t> rp, rc;
    std::vector<uint8_t> rv;
    for (int k = 0; k < 2; k++) {
      zcsr(re[k], d, rp, rc, rv);
      OG_REQUIRE(rp == rows.ptr[k] && rc == rows.col[k] && rv == rows.val[k], who + std::string(": the .r1cs is not this key's circuit (matrix ") + (k ? "B" : "A") + " differs)");
    }
    zcsr(re[2], d, rows.ptr[2], rows.col[2], rows.val[2]);
    flags = 0;
  }
  // ---- points
  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev dev;
  const size_t n1 = 3 + (l + 1) + m + m + nl, n2 = 3 + m;
  std::vector<uint8_t> g1_in(n1 * 64), g1(n1 * 64), g2_in(n2 * 128), g2(n2 * 128), hq((d - 1) * 64);
  {
    uint8_t* o = g1_in.data();
    memcpy(o, h + 84, 64); o += 64;                      // alpha1
    memcpy(o, h + 84 + 64, 64); o += 64;                 // beta1
    memcpy(o, h + 84 + 64 + 64 + 128 + 128, 64); o += 64;  // delta1
    for (uint32_t id : {3u, 5u, 6u, 8u}) {
      memcpy(o, bf.sec[id].first, bf.sec[id].second);
      o += bf.sec[id].second;
    }
    uint8_t* q = g2_in.data();
    memcpy(q, h + 84 + 128, 128); q += 128;        // beta2
    memcpy(q, h + 84 + 128 + 128, 128); q += 128;  // gamma2
    memcpy(q, h + 84 + 128 + 256 + 64, 128); q += 128;  // delta2
    memcpy(q, bf.sec[7].first, bf.sec[7].second);
  }
  OG_TRY(lem_convert(ctx, dev, false, false, g1_in.data(), n1, g1.data(), nullptr, who));
  OG_TRY(lem_convert(ctx, dev, true, false, g2_in.data(), n2, g2.data(), nullptr, who));
  {  // the H section -> the coefficient-basis H query
    uint8_t* hm_d;
    OG_TRY(dev.get(d * 64, &hm_d));
    std::vector<uint8_t> h_in(bf.sec[9].first, bf.sec[9].first + d * 64), h_canon(d * 64), tw, post;
    OG_TRY(lem_convert(ctx, dev, false, false, h_in.data(), d, h_canon.data(), hm_d, who));
    pow_table(dom.w, Fr::one(), d / 2, tw);
    const Fr two = fe_dbl(Fr::one());
    pow_table(dom.psi, fe_neg(two), d, post);
    OG_TRY(ecntt_g1(ctx, dev, hm_d, z.power, tw, nullptr, &post, d - 1, hq.data()));
  }
  const uint8_t* ic = &g1[192];
  KeyParts parts;
  parts.m = m; parts.l = l; parts.log_d = z.power; parts.n_rows = d; parts.flags = flags;
  parts.alpha1 = &g1[0]; parts.beta1 = &g1[64]; parts.delta1 = &g1[128];
  parts.beta2 = &g2[0]; parts.gamma2 = &g2[128]; parts.delta2 = &g2[256];
  parts.ic = ic;
  parts.query[0] = ic + (l + 1) * 64; parts.query[1] = parts.query[0] + m * 64; parts.query[2] = &g2[384];
  parts.query[3] = parts.query[1] + m * 64; parts.query[4] = hq.data();
  key_blobs(parts, rows, pk, vk);
  return OG_OK;
}

// The way back: this library's key as a .zkey snarkjs can prove with.  The C matrix stays behind (the format has no room for it:
// snarkjs' prover takes C z = (A z) o (B z), which is C z for every satisfying witness); the H section is the inverse transform
//   H'[i] = 1/d sum_j w^(-i j) (-2 psi^j)^-1 H[j],   H[d - 1] := the point at infinity
// (the quotient has degree <= d - 2, so its d-th coefficient never meets a base); section 10 says "no contributions".
static int zkey_export(og_ctx* ctx, const uint8_t* pkb, size_t pk_len, const uint8_t* vkb, size_t vk_len, std::vector<uint8_t>& out) {
  const std::string who = "og_zkey_export";
  PkView pv;
  VkView vv;
  OG_TRY(pk_view(pkb, pk_len, who, &pv));  // (header words 8 and 9 are not looked at, nor is the C matrix: neither goes into the file)
  const uint64_t m = pv.m, l = pv.l, power = pv.log_d, n_rows = pv.n_rows, d = pv.d, nl = pv.nl, nh = pv.nh;
  OG_REQUIRE(power <= 27, who + ": bad key header (a .zkey's domain holds at most 2^27 points)");
  OG_TRY(vk_view(vkb, vk_len, who, &vv));
  OG_REQUIRE(vk_is_of_pk(vv, pv), who + ": the verifying key does not belong to this proving key (n_pub, alpha, beta or delta differ)");
  OG_TRY(pk_csr_check(pv, 2, who));
  const uint8_t* const* q_h = pv.query;
  ZDomain dom;
  OG_TRY(zdomain((int)power, who, &dom));
  // ---- coefficients: row i -> constraint i k mod d, value x 2^512
  Fr r2 = Fr::one();
  for (int i = 0; i < 512; i++) r2 = fe_dbl(r2);
  std::vector<uint8_t> cs(4);
  uint64_t n_coef = 0;
  for (int k = 0; k < 2; k++) {
    for (uint64_t row = 0; row < n_rows; row++) {
      for (uint32_t e = rd32(pv.ptr[k] + row * 4), end = rd32(pv.ptr[k] + row * 4 + 4); e < end; e++) {
        const Fr v = zfr_load(pv.val[k] + (size_t)e * 32);
        OG_REQUIRE(fe_lt_modulus(v), who + ": coefficient not canonical");
        const uint32_t rec[3] = {(uint32_t)k, (uint32_t)((row * dom.k) & (d - 1)), rd32(pv.col[k] + (size_t)e * 4)};
        cs.insert(cs.end(), (const uint8_t*)rec, (const uint8_t*)rec + 12);
        cs.resize(cs.size() + 32);
        zfr_store(&cs[cs.size() - 32], fe_from_mont(fe_mul(fe_to_mont(v), r2)));
        n_coef++;
      }
    }
  }
  OG_REQUIRE(n_coef < (1ull << 32), who + ": too many coefficients");
  const uint32_t n_coef32 = (uint32_t)n_coef;
  memcpy(cs.data(), &n_coef32, 4);
  // ---- points
  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev dev;
  const size_t n1 = 3 + (l + 1) + m + m + nl, n2 = 3 + m;
  std::vector<uint8_t> g1_in(n1 * 64), g1(n1 * 64), g2_in(n2 * 128), g2(n2 * 128), hsec(d * 64);
  {
    uint8_t* o = g1_in.data();
    memcpy(o, pv.alpha1, 64); o += 64;
    memcpy(o, pv.beta1, 64); o += 64;
    memcpy(o, pv.delta1, 64); o += 64;
    memcpy(o, vv.ic, (l + 1) * 64); o += (l + 1) * 64;
    memcpy(o, q_h[0], m * 64); o += m * 64;
    memcpy(o, q_h[1], m * 64); o += m * 64;
    memcpy(o, q_h[3], nl * 64);
    uint8_t* q = g2_in.data();
    memcpy(q, pv.beta2, 128); q += 128;
    memcpy(q, vv.gamma2, 128); q += 128;
    memcpy(q, pv.delta2, 128); q += 128;
    memcpy(q, q_h[2], m * 128);
  }
  OG_TRY(lem_convert(ctx, dev, false, true, g1_in.data(), n1, g1.data(), nullptr, who));
  OG_TRY(lem_convert(ctx, dev, true, true, g2_in.data(), n2, g2.data(), nullptr, who));
  {
    uint8_t* hm_d;
    OG_TRY(dev.get(d * 64, &hm_d));
    std::vector<uint8_t> h_in(d * 64, 0), h_file(d * 64), h_canon(d * 64), tw, pre;
    memcpy(h_in.data(), q_h[4], nh * 64);  // H[d - 1] = infinity
    OG_TRY(lem_convert(ctx, dev, false, true, h_in.data(), d, h_file.data(), hm_d, who));  // (only the Montgomery copy on the device is used)
    pow_table(fe_inv(dom.w), Fr::one(), d / 2, tw);
    Fr nn = Fr::one();  // d as a field element: 2^power
    for (uint64_t i = 0; i < power; i++) nn = fe_dbl(nn);
    const Fr two = fe_dbl(Fr::one());
    pow_table(fe_inv(dom.psi), fe_inv(fe_mul(fe_neg(two), nn)), d, pre);  // (-2 psi^j)^-1 / d
    OG_TRY(ecntt_g1(ctx, dev, hm_d, (int)power, tw, &pre, nullptr, d, h_canon.data()));
    OG_TRY(lem_convert(ctx, dev, false, true, h_canon.data(), d, hsec.data(), nullptr, who));
  }
  // ---- the file
  out.clear();
  auto put32 = [&](uint32_t v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); };
  auto put64 = [&](uint64_t v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + 8); };
  auto section = [&](uint32_t id, const std::vector<uint8_t>& body) {
    put32(id);
    put64(body.size());
    out.insert(out.end(), body.begin(), body.end());
  };
  out.insert(out.end(), (const uint8_t*)"zkey", (const uint8_t*)"zkey" + 4);
  put32(1);
  put32(10);
  const uint8_t *alpha1 = &g1[0], *beta1 = &g1[64], *delta1 = &g1[128], *ic = &g1[192];
  const uint8_t *aq = ic + (l + 1) * 64, *b1q = aq + m * 64, *cq = b1q + m * 64;
  const uint8_t *beta2 = &g2[0], *gamma2 = &g2[128], *delta2 = &g2[256], *b2q = &g2[384];
  section(1, {1, 0, 0, 0});
  {
    std::vector<uint8_t> hdr;
    auto h32 = [&](uint32_t v) { hdr.insert(hdr.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); };
    auto hb = [&](const uint8_t* p, size_t n) { hdr.insert(hdr.end(), p, p + n); };
    h32(32); hb(FQ_BYTES, 32); h32(32); hb(FR_BYTES, 32);
    h32((uint32_t)m); h32((uint32_t)l); h32((uint32_t)d);
    hb(alpha1, 64); hb(beta1, 64); hb(beta2, 128); hb(gamma2, 128); hb(delta1, 64); hb(delta2, 128);
    section(2, hdr);
  }
  section(3, std::vector<uint8_t>(ic, ic + (l + 1) * 64));
  section(4, cs);
  section(5, std::vector<uint8_t>(aq, aq + m * 64));
  section(6, std::vector<uint8_t>(b1q, b1q + m * 64));
  section(7, std::vector<uint8_t>(b2q, b2q + m * 128));
  section(8, std::vector<uint8_t>(cq, cq + nl * 64));
  section(9, hsec);
  section(10, std::vector<uint8_t>(68, 0));  // circuit hash (zeros: not snarkjs' hash of a .r1cs) | 0 contributions
  return OG_OK;
}

}  // namespace og

using namespace og;

extern "C" {

int og_zkey_import(og_ctx* ctx, const uint8_t* zkey, size_t zkey_len, const og_r1cs* r1cs, uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out,
                   size_t* vk_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && zkey && pk_out && pk_len && vk_out && vk_len, "og_zkey_import: null argument");
    *pk_out = *vk_out = nullptr;
    *pk_len = *vk_len = 0;
    std::vector<uint8_t> pk, vk;
    OG_TRY(zkey_import(ctx, zkey, zkey_len, r1cs, pk, vk));
    uint8_t *a = nullptr, *b = nullptr;
    size_t al = 0, bl = 0;
    OG_TRY(blob_out(pk, &a, &al, "og_zkey_import"));
    if (blob_out(vk, &b, &bl, "og_zkey_import") != OG_OK) {
      free(a);
      return OG_ERR_INVALID;
    }
    *pk_out = a; *pk_len = al;
    *vk_out = b; *vk_len = bl;
    return OG_OK;
  });
}

int og_zkey_export(og_ctx* ctx, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, uint8_t** zkey_out, size_t* zkey_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && pk && vk && zkey_out && zkey_len, "og_zkey_export: null argument");
    *zkey_out = nullptr;
    *zkey_len = 0;
    std::vector<uint8_t> z;
    OG_TRY(zkey_export(ctx, pk, pk_len, vk, vk_len, z));
    return blob_out(z, zkey_out, zkey_len, "og_zkey_export");
  });
}

// circom's .r1cs (iden3 r1csfile): magic "r1cs", version 1; section 1 = u32 n8 | prime | u32 nWires | u32 nPubOut | u32 nPubIn |
// u32 nPrvIn | u64 nLabels | u32 mConstraints; section 2 = per constraint three linear combinations A, B, C, each u32 n followed
// by n x (u32 wire | n8-byte little-endian NORMAL-form coefficient); section 3 (wire -> label) is not needed here.
// Wires: 0 = the constant 1, then the public outputs, the public inputs (n_pub = nPubOut + nPubIn), the rest.
int og_r1cs_read(const uint8_t* file, size_t len, og_r1cs** out) {
  return guarded([&]() -> int {
    OG_REQUIRE(file && out, "og_r1cs_read: null argument");
    *out = nullptr;
    BinFile bf;
    OG_TRY(binfile_parse(file, len, "r1cs", 1, "og_r1cs_read", &bf));
    OG_REQUIRE(bf.sec.count(1) && bf.sec.count(2), "og_r1cs_read: section missing");
    const uint8_t* h = bf.sec[1].first;
    OG_REQUIRE(bf.sec[1].second == 4 + 32 + 16 + 8 + 4 && rd32(h) == 32 && memcmp(h + 4, FR_BYTES, 32) == 0, "og_r1cs_read: not BN254's scalar field");
    const uint64_t n_wires = rd32(h + 36), n_pub = (uint64_t)rd32(h + 40) + rd32(h + 44), nc = rd32(h + 60);
    OG_REQUIRE(n_wires >= 1 && n_pub < n_wires && n_wires < (1ull << 31) && nc < (1ull << 31), "og_r1cs_read: bad sizes");
    std::unique_ptr<og_r1cs> r(new og_r1cs());
    r->n_wires = n_wires; r->n_pub = n_pub; r->n_constraints = nc;
    const uint8_t* p = bf.sec[2].first;
    const uint8_t* end = p + bf.sec[2].second;
    for (int k = 0; k < 3; k++) r->ptr[k].push_back(0);
    for (uint64_t c = 0; c < nc; c++)
      for (int k = 0; k < 3; k++) {
        OG_REQUIRE(end - p >= 4, "og_r1cs_read: constraint section truncated");
        const uint64_t n = rd32(p);
        p += 4;
        OG_REQUIRE((uint64_t)(end - p) >= n * 36, "og_r1cs_read: constraint section truncated");
        for (uint64_t i = 0; i < n; i++, p += 36) {
          const uint32_t w = rd32(p);
          OG_REQUIRE(w < n_wires && fe_lt_modulus(zfr_load(p + 4)), "og_r1cs_read: constraint " + std::to_string(c) + " holds a wire or a coefficient out of range");
          r->col[k].push_back(w);
          r->val[k].insert(r->val[k].end(), p + 4, p + 36);
        }
        OG_REQUIRE(r->col[k].size() < (1ull << 32), "og_r1cs_read: too many coefficients");
        r->ptr[k].push_back((uint32_t)r->col[k].size());
      }
    OG_REQUIRE(p == end, "og_r1cs_read: bytes left over after the last constraint");
    *out = r.release();
    return OG_OK;
  });
}

int og_r1cs_write(const og_r1cs* r, uint8_t** file_out, size_t* file_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(r && file_out && file_len, "og_r1cs_write: null argument");
    *file_out = nullptr;
    *file_len = 0;
    std::vector<uint8_t> out, body;
    auto put32 = [](std::vector<uint8_t>& v, uint32_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); };
    auto put64 = [](std::vector<uint8_t>& v, uint64_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 8); };
    for (uint64_t c = 0; c < r->n_constraints; c++)
      for (int k = 0; k < 3; k++) {
        put32(body, r->ptr[k][c + 1] - r->ptr[k][c]);
        for (uint32_t e = r->ptr[k][c]; e < r->ptr[k][c + 1]; e++) {
          put32(body, r->col[k][e]);
          body.insert(body.end(), &r->val[k][(size_t)e * 32], &r->val[k][(size_t)e * 32] + 32);
        }
      }
    out.insert(out.end(), (const uint8_t*)"r1cs", (const uint8_t*)"r1cs" + 4);
    put32(out, 1); put32(out, 3);
    put32(out, 1); put64(out, 64);
    put32(out, 32);
    out.insert(out.end(), FR_BYTES, FR_BYTES + 32);
    put32(out, (uint32_t)r->n_wires); put32(out, 0); put32(out, (uint32_t)r->n_pub); put32(out, (uint32_t)(r->n_wires - r->n_pub - 1));  // (every public wire as an input)
    put64(out, r->n_wires); put32(out, (uint32_t)r->n_constraints);
    put32(out, 2); put64(out, body.size());
    out.insert(out.end(), body.begin(), body.end());
    put32(out, 3); put64(out, r->n_wires * 8);
    for (uint64_t w = 0; w < r->n_wires; w++) put64(out, w);  // wire -> label: the identity
    return blob_out(out, file_out, file_len, "og_r1cs_write");
  });
}

int og_wtns_read(const uint8_t* wtns, size_t len, uint8_t* values_out, size_t capacity, uint64_t* n_out) {
  return guarded([&]() -> int {
    OG_REQUIRE(wtns && n_out, "og_wtns_read: null argument");
    *n_out = 0;
    BinFile bf;
    OG_TRY(binfile_parse(wtns, len, "wtns", 2, "og_wtns_read", &bf));
    OG_REQUIRE(bf.sec.count(1) && bf.sec.count(2), "og_wtns_read: section missing");
    const uint8_t* h = bf.sec[1].first;
    OG_REQUIRE(bf.sec[1].second == 40 && rd32(h) == 32 && memcmp(h + 4, FR_BYTES, 32) == 0, "og_wtns_read: not BN254's scalar field");
    const uint64_t n = rd32(h + 36);
    OG_REQUIRE(bf.sec[2].second == n * 32, "og_wtns_read: witness section length does not match its count");
    *n_out = n;
    if (!values_out) return OG_OK;  // (a size query)
    OG_REQUIRE(capacity >= n, "og_wtns_read: the output holds " + std::to_string(capacity) + " values, the file " + std::to_string(n));
    for (uint64_t i = 0; i < n; i++)
      OG_REQUIRE(fe_lt_modulus(zfr_load(bf.sec[2].first + i * 32)), "og_wtns_read: value " + std::to_string(i) + " is not below the modulus");
    memcpy(values_out, bf.sec[2].first, n * 32);
    return OG_OK;
  });
}

int og_wtns_write(const uint8_t* values, uint64_t n, uint8_t** wtns_out, size_t* wtns_len) {
  return guarded([&]() -> int {
    OG_REQUIRE((values || n == 0) && wtns_out && wtns_len && n < (1ull << 32), "og_wtns_write: bad argument");
    *wtns_out = nullptr;
    *wtns_len = 0;
    for (uint64_t i = 0; i < n; i++) OG_REQUIRE(fe_lt_modulus(zfr_load(values + i * 32)), "og_wtns_write: value " + std::to_string(i) + " is not canonical");
    std::vector<uint8_t> out;
    auto put32 = [&](uint32_t v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); };
    auto put64 = [&](uint64_t v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + 8); };
    out.insert(out.end(), (const uint8_t*)"wtns", (const uint8_t*)"wtns" + 4);
    put32(2); put32(2);
    put32(1); put64(40);
    put32(32);
    out.insert(out.end(), FR_BYTES, FR_BYTES + 32);
    put32((uint32_t)n);
    put32(2); put64(n * 32);
    out.insert(out.end(), values, values + n * 32);
    return blob_out(out, wtns_out, wtns_len, "og_wtns_write");
  });
}

}  // extern "C"
