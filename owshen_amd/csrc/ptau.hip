// Groth16 key generation from a powers-of-tau file: `snarkjs groth16 setup` on the GPU (og_setup_ptau), the one-scalar delta
// step of phase 2 (og_pk_contribute), a host-only look at a .ptau's header (og_ptau_info), and the two checks that go with
// them: is a file a ceremony (og_ptau_verify), is a key this circuit's key from this ceremony (og_pk_verify) -- at the end.
//
// No reference counterpart: the snapshot holds no prover and no key.  og_setup (keygen.hip) takes the toxic
// waste as plain scalars, which is good for tests and benchmarks only; here no secret scalar is ever in the process -- the
// file holds tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1 and beta G2, and everything a key needs is linear in those:
//
//   * Lagrange bases as points.  L_row(tau) P = 1/d sum_j w^(-row j) tau^j P over THIS library's root w = 7^((r-1)/d) (the row
//     order of og_setup / og_lagrange_evals_d: no permutation): an inverse DFT of size d over the points of sections 2, 4, 5
//     (G1) and 3 (G2), the kernels of snarkfile.hip.h written once over the group law.
//   * The transposed sparse product over points.  Query entry of wire i = sum over the non-zeros of column i of
//     val[e] Lag[row[e]] (the input-consistency rows included as keygen.hip appends them): A and B over the tau basis give
//     the A / B1 / B2 queries, beta-basis A + alpha-basis B + tau-basis C gives kk_i = IC (i <= n_pub) or L.  One lane per
//     NON-ZERO forms its term (coefficients 1 and r - 1 skip the multiplication, any other runs double-and-add from its top
//     bit), then a segmented sum in levels of at most SPMV_SEG terms per lane: wire 0 of the withdraw circuit holds tens of thousands
//     of terms, and no lane ever walks more than SPMV_SEG of them.
//   * H query: tau^j Z(tau) G1 = tau^(j+d) G1 - tau^j G1 at delta = 1: one subtraction per entry, no transform.
//
// The result is og_setup(r1cs, tau, alpha, beta, gamma = 1, delta = 1) byte for byte (canonical affine output does not depend
// on the path taken), which is what the tests pin; og_pk_contribute(d') then gives og_setup(.., 1, d').
//
// The file format is written down from snarkjs' published sources (powersoftau_new.js / binfileutils); no file made by snarkjs
// itself was available to test against.  Whether the file is a VALID ceremony (the geometric-sequence
// pairing checks) is not og_setup_ptau's business -- og_ptau_verify below asks that; what og_setup_ptau checks on every point
// it uses: coordinates < q, on the curve, tauG1[0] / tauG2[0] the generators, G2 points in the order-r subgroup.
#include "ctx.h"
#include "field.hip.h"
#include "ec.hip.h"
#include "snarkfile.hip.h"
#include "point_spmv.hip.h"
#include "keygen.h"
#include "key_blob.h"
#include "mimc7.hip.h"
#include "msm.hip.h"
#include "prover.h"
#include "verify_tower.h"
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace og {

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// flags[0] |= 4: [order] P != infinity for some point (affine Montgomery; infinity itself passes).  A lane per point.
__global__ void __launch_bounds__(64) k_g2_subgroup(const uint8_t* __restrict__ aff, size_t n, K256 order, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G2XYZZ p = G2XYZZ::from_affine(G2Affine::load(aff + i * 128));
  const G2XYZZ q = ecntt_smul(p, order);
  if (!q.is_inf()) atomicOr(flags, 4u);
}

// out[j] = tau[j + d] - tau[j], j < d - 1 (tau: affine Montgomery, out: canonical)
__global__ void __launch_bounds__(64) k_ptau_h(const uint8_t* __restrict__ tau, size_t d, uint8_t* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j + 1 >= d) return;
  const G1XYZZ hi = G1XYZZ::from_affine(G1Affine::load(tau + (j + d) * 64));
  G1Affine a = xyzz_to_affine(xyzz_madd_signed(hi, G1Affine::load(tau + j * 64), true));
  a.x = fe_from_mont(a.x);
  a.y = fe_from_mont(a.y);
  a.store(out + j * 64);
}

// out[i] = k . in[i], canonical affine in and out, ONE scalar for every lane (the wave does not diverge).  b: the curve's
// constant in Montgomery form.  flags[0] |= 1: a coordinate >= q; |= 2: a point off the curve.
template <class T>
__global__ void __launch_bounds__(64) k_smul_uniform(const uint8_t* __restrict__ in, size_t n, K256 k, const uint8_t* __restrict__ b_mont,
                                                    uint8_t* __restrict__ out, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<T> c = Affine<T>::load(in + i * Affine<T>::BYTES);
  Affine<T> r = Affine<T>::inf();
  if (lem_or(c.x) | lem_or(c.y)) {
    if (!lem_lt(c.x) || !lem_lt(c.y)) {
      atomicOr(flags, 1u);
    } else {
      const Affine<T> m = {FieldIO<T>::to_mont(c.x), FieldIO<T>::to_mont(c.y)};
      const T b = FieldIO<T>::load(b_mont);
      if (!(f_sqr(m.y) == f_add(f_mul(f_sqr(m.x), m.x), b))) atomicOr(flags, 2u);
      r = xyzz_to_affine(ecntt_smul(XYZZ<T>::from_affine(m), k));
      r.x = FieldIO<T>::from_mont(r.x);
      r.y = FieldIO<T>::from_mont(r.y);
    }
  }
  r.store(out + i * Affine<T>::BYTES);
}

// The challenge scalars of og_ptau_verify / og_pk_verify: out[i] = the low 128 bits of MiMC7 hash2(seed, section 2^32 + i), a
// lane per scalar, as the 32-byte canonical scalars the digit sort reads.  seed: 32 B canonical, on the device.
__global__ void __launch_bounds__(128) k_challenge_scalars(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ seed, uint32_t section,
                                                          size_t n, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx[8] = {(uint32_t)i, section, 0, 0, 0, 0, 0, 0};
  const Fr h = fe_from_mont(mimc7_hash2<false>(consts, fe_to_mont(fe_load<FrParams>(seed)), fe_to_mont(fe_from_words<FrParams>(idx))));
  uint32_t w[8];
  fe_to_words(w, h);
  uint4* q = reinterpret_cast<uint4*>(out + i * 32);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(0, 0, 0, 0);
}

// Canonical affine points (a key's bytes) -> affine Montgomery, checked: flags[0] |= 1: a coordinate >= q; |= 2: a point off
// the curve (such an entry is stored as infinity: nothing after this kernel meets a point outside the curve).  b: the
// curve's constant in Montgomery form.  All zeros is the point at infinity, on both sides.
template <class T>
__global__ void __launch_bounds__(256) k_canon_to_mont(const uint8_t* __restrict__ in, size_t n, const uint8_t* __restrict__ b_mont,
                                                      uint8_t* __restrict__ out_mont, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<T> c = Affine<T>::load(in + i * Affine<T>::BYTES);
  Affine<T> m = Affine<T>::inf();
  if (lem_or(c.x) | lem_or(c.y)) {
    if (!lem_lt(c.x) || !lem_lt(c.y)) {
      atomicOr(flags, 1u);
    } else {
      m = {FieldIO<T>::to_mont(c.x), FieldIO<T>::to_mont(c.y)};
      const T b = FieldIO<T>::load(b_mont);
      if (!(f_sqr(m.y) == f_add(f_mul(f_sqr(m.x), m.x), b))) {
        atomicOr(flags, 2u);
        m = Affine<T>::inf();
      }
    }
  }
  m.store(out_mont + i * Affine<T>::BYTES);
}

// ---- the file -----------------------------------------------------------------------------------------------------------------
static const char* const PTAU_SEC[7] = {"", "section 1 (header)", "section 2 (tauG1)", "section 3 (tauG2)", "section 4 (alphaTauG1)", "section 5 (betaTauG1)",
                                        "section 6 (betaG2)"};

struct PtauHeader {
  uint32_t power = 0, ceremony_power = 0;
};

static int ptau_parse(const uint8_t* data, size_t len, const std::string& who, BinFile* bf, PtauHeader* hd) {
  OG_TRY(binfile_parse(data, len, "ptau", 1, who, bf));
  OG_REQUIRE(bf->sec.count(1), who + ": " + PTAU_SEC[1] + " missing");
  const uint8_t* h = bf->sec[1].first;
  OG_REQUIRE(bf->sec[1].second == 4 + 32 + 8 && rd32(h) == 32, who + ": " + PTAU_SEC[1] + " has the wrong length for a 32-byte base field");
  OG_REQUIRE(memcmp(h + 4, FQ_BYTES, 32) == 0, who + ": " + PTAU_SEC[1] + ": the base field is not BN254's");
  hd->power = rd32(h + 36);
  hd->ceremony_power = rd32(h + 40);
  OG_REQUIRE(hd->power <= 28 && hd->ceremony_power <= 28 && hd->power <= hd->ceremony_power, who + ": " + PTAU_SEC[1] + ": bad power " +
                                                                                               std::to_string(hd->power) + " / " + std::to_string(hd->ceremony_power));
  return OG_OK;
}

// ---- device steps ---------------------------------------------------------------------------------------------------------
// `n` points of section `sec` -> canonical on the host, Montgomery on the device (mont_d: n_dev >= n slots, the rest infinity)
static int ptau_decode(og_ctx* ctx, ZDev& dev, BinFile& bf, int sec, bool g2, size_t n, size_t n_dev, std::vector<uint8_t>& canon, uint8_t** mont_d,
                       const std::string& who) {
  const size_t pb = g2 ? 128 : 64;
  std::vector<uint8_t> in(n_dev * pb, 0);
  memcpy(in.data(), bf.sec[sec].first, n * pb);
  canon.resize(n_dev * pb);
  OG_TRY(dev.get(n_dev * pb, mont_d));
  return lem_convert(ctx, dev, g2, false, in.data(), n_dev, canon.data(), *mont_d, who + ": " + PTAU_SEC[sec]);
}

// *outside = 1 if some point of the n (affine Montgomery, device) is not in the order-r subgroup
static int g2_subgroup_flags(og_ctx* ctx, ZDev& dev, const uint8_t* mont_d, size_t n, bool* outside) {
  uint8_t* f_d;
  OG_TRY(dev.get(4, &f_d));
  OG_HIP(hipMemsetAsync(f_d, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_g2_subgroup, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, mont_d, n, fr_order_k256(0), (uint32_t*)f_d);
  OG_HIP(hipGetLastError());
  uint32_t flags = 0;
  OG_HIP(hipMemcpyAsync(&flags, f_d, 4, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  *outside = flags != 0;
  return OG_OK;
}

static int g2_subgroup_check(og_ctx* ctx, ZDev& dev, const uint8_t* mont_d, size_t n, const std::string& who_sec) {
  bool outside = false;
  OG_TRY(g2_subgroup_flags(ctx, dev, mont_d, n, &outside));
  OG_REQUIRE(!outside, who_sec + ": a point is not in the order-r subgroup");
  return OG_OK;
}

// sections 2..6 are present and have the lengths the header's power asks for
static int ptau_sections(BinFile& bf, const PtauHeader& hd, const std::string& who) {
  const uint64_t np = 1ull << hd.power;
  const uint64_t want[7] = {0, 0, (2 * np - 1) * 64, np * 128, np * 64, np * 64, 128};
  for (uint32_t id = 2; id <= 6; id++) {
    OG_REQUIRE(bf.sec.count(id), who + ": " + PTAU_SEC[id] + " missing");
    OG_REQUIRE(bf.sec[id].second == want[id], who + ": " + PTAU_SEC[id] + " has " + std::to_string(bf.sec[id].second) + " bytes, power " +
                                                  std::to_string(hd.power) + " asks for " + std::to_string(want[id]));
  }
  return OG_OK;
}

// who: the entry point the reasons name (og_setup_ptau, or og_pk_verify rebuilding the delta = 1 key)
static int ptau_setup(og_ctx* ctx, const og_r1cs* r, const uint8_t* data, size_t len, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk,
               const std::string& who = "og_setup_ptau") {
  BinFile bf;
  PtauHeader hd;
  OG_TRY(ptau_parse(data, len, who, &bf, &hd));
  OG_TRY(ptau_sections(bf, hd, who));
  QapRows rows;
  OG_TRY(r1cs_qap_rows(r, who, &rows));
  const size_t m = r->n_wires, l = r->n_pub, n_rows = r->n_constraints + l + 1;
  int log_d = 1;
  while (((size_t)1 << log_d) < n_rows) log_d++;
  OG_REQUIRE(log_d <= 28, who + ": too many constraints for the 2^28 domain");
  OG_REQUIRE((uint32_t)log_d <= hd.power, who + ": " + PTAU_SEC[1] + ": power " + std::to_string(hd.power) + " is below the circuit's domain 2^" +
                                              std::to_string(log_d));
  const size_t d = (size_t)1 << log_d, nh = d - 1;
  std::vector<uint32_t> tptr[3], trow[3];
  std::vector<uint8_t> tval[3];
  for (int k = 0; k < 3; k++) csr_transpose(rows.ptr[k], rows.col[k], rows.val[k], n_rows, m, tptr[k], trow[k], tval[k]);

  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev dev;
  // ---- decode and check every point that is used
  std::vector<uint8_t> tau_c, alpha_c, beta_c, tau2_c, beta2_c;
  uint8_t *tau_m, *alpha_m, *beta_m, *tau2_m, *beta2_m;
  OG_TRY(ptau_decode(ctx, dev, bf, 2, false, 2 * d - 1, 2 * d, tau_c, &tau_m, who));
  OG_REQUIRE(memcmp(tau_c.data(), G1_GEN_BYTES, 64) == 0, who + ": " + PTAU_SEC[2] + ": the first point is not the G1 generator");
  OG_TRY(ptau_decode(ctx, dev, bf, 3, true, d, d, tau2_c, &tau2_m, who));
  OG_REQUIRE(memcmp(tau2_c.data(), G2_GEN_BYTES, 128) == 0, who + ": " + PTAU_SEC[3] + ": the first point is not the G2 generator");
  OG_TRY(ptau_decode(ctx, dev, bf, 4, false, d, d, alpha_c, &alpha_m, who));
  OG_TRY(ptau_decode(ctx, dev, bf, 5, false, d, d, beta_c, &beta_m, who));
  OG_TRY(ptau_decode(ctx, dev, bf, 6, true, 1, 1, beta2_c, &beta2_m, who));
  OG_TRY(g2_subgroup_check(ctx, dev, tau2_m, d, who + ": " + PTAU_SEC[3]));
  OG_TRY(g2_subgroup_check(ctx, dev, beta2_m, 1, who + ": " + PTAU_SEC[6]));
  // ---- Lagrange bases as points: lag1 = tau | alpha | beta (d each), lag2 = tau in G2; affine Montgomery
  const FfRoots& f = ff_roots();
  OG_REQUIRE(f.ok, who + ": internal: the roots of unity are not what the field layer expects");
  std::vector<uint8_t> tw, post(32);
  pow_table(fe_inv(zfr_pow2k(f.w28_own, 28 - log_d)), Fr::one(), d / 2, tw);
  Fr nn = Fr::one();  // d as a field element
  for (int i = 0; i < log_d; i++) nn = fe_dbl(nn);
  zfr_store(post.data(), fe_from_mont(fe_inv(nn)));
  uint8_t *lag1_d, *lag2_d;
  OG_TRY(dev.get(3 * d * 64, &lag1_d));
  OG_TRY(dev.get(d * 128, &lag2_d));
  OG_TRY(ecntt_run<Fq>(ctx, dev, tau_m, log_d, tw, nullptr, &post, true, d, lag1_d, true));
  OG_TRY(ecntt_run<Fq>(ctx, dev, alpha_m, log_d, tw, nullptr, &post, true, d, lag1_d + d * 64, true));
  OG_TRY(ecntt_run<Fq>(ctx, dev, beta_m, log_d, tw, nullptr, &post, true, d, lag1_d + 2 * d * 64, true));
  OG_TRY(ecntt_run<Fq2>(ctx, dev, tau2_m, log_d, tw, nullptr, &post, true, d, lag2_d, true));
  // ---- the queries
  uint8_t *a_d, *b1_d, *b2_d, *kk_d, *h_d;
  OG_TRY(dev.get(m * 64, &a_d));
  OG_TRY(dev.get(m * 64, &b1_d));
  OG_TRY(dev.get(m * 128, &b2_d));
  OG_TRY(dev.get(m * 64, &kk_d));
  OG_TRY(dev.get(nh * 64, &h_d));
  OG_TRY(point_spmv<Fq>(ctx, lag1_d, tptr[0], trow[0], tval[0], m, a_d));
  OG_TRY(point_spmv<Fq>(ctx, lag1_d, tptr[1], trow[1], tval[1], m, b1_d));
  OG_TRY(point_spmv<Fq2>(ctx, lag2_d, tptr[1], trow[1], tval[1], m, b2_d));
  {  // kk_i: wire i's entries of A over the beta basis, of B over the alpha basis, of C over the tau basis
    const size_t nnz = trow[0].size() + trow[1].size() + trow[2].size();
    OG_REQUIRE(3 * (uint64_t)d < (1ull << 32) && nnz < (1ull << 32), who + ": circuit too large");
    std::vector<uint32_t> kptr(m + 1, 0), kidx;
    std::vector<uint8_t> kval;
    kidx.reserve(nnz);
    kval.reserve(nnz * 32);
    const uint32_t base[3] = {(uint32_t)(2 * d), (uint32_t)d, 0};
    for (size_t i = 0; i < m; i++) {
      for (int k = 0; k < 3; k++) {
        for (uint32_t e = tptr[k][i]; e < tptr[k][i + 1]; e++) kidx.push_back(base[k] + trow[k][e]);
        kval.insert(kval.end(), tval[k].begin() + (size_t)tptr[k][i] * 32, tval[k].begin() + (size_t)tptr[k][i + 1] * 32);
      }
      kptr[i + 1] = (uint32_t)kidx.size();
    }
    OG_TRY(point_spmv<Fq>(ctx, lag1_d, kptr, kidx, kval, m, kk_d));
  }
  hipLaunchKernelGGL(k_ptau_h, dim3(grid_for(d, 64)), dim3(64), 0, ctx->stream, tau_m, d, h_d);
  OG_HIP(hipGetLastError());
  std::vector<uint8_t> a_q(m * 64), b1_q(m * 64), b2_q(m * 128), kk(m * 64), h_q(nh * 64);
  OG_HIP(hipMemcpyAsync(a_q.data(), a_d, m * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(b1_q.data(), b1_d, m * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(b2_q.data(), b2_d, m * 128, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(kk.data(), kk_d, m * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(h_q.data(), h_d, nh * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  // ---- gamma = delta = 1: IC = kk[0 .. l], L = kk[l + 1 ..], gamma2 = delta2 = the G2 generator, delta1 = the G1 generator
  KeyParts parts;
  parts.m = m; parts.l = l; parts.log_d = log_d; parts.n_rows = n_rows;
  parts.alpha1 = alpha_c.data(); parts.beta1 = beta_c.data(); parts.delta1 = G1_GEN_BYTES;
  parts.beta2 = beta2_c.data(); parts.gamma2 = G2_GEN_BYTES; parts.delta2 = G2_GEN_BYTES;
  parts.query[0] = a_q.data(); parts.query[1] = b1_q.data(); parts.query[2] = b2_q.data();
  parts.query[3] = kk.data() + (l + 1) * 64; parts.query[4] = h_q.data();
  parts.ic = kk.data();
  key_blobs(parts, rows, pk, vk);
  return OG_OK;
}

// ---- the delta step ---------------------------------------------------------------------------------------------------------
template <class T>
static int smul_uniform(og_ctx* ctx, ZDev& dev, const uint8_t* in, size_t n, const K256& k, uint8_t* out, const std::string& who) {
  if (n == 0) return OG_OK;
  uint32_t flags = 0;
  OG_TRY(lem_run(ctx, dev, Affine<T>::BYTES == 128, false, in, n, out, nullptr, &flags, [&](uint8_t* in_d, uint8_t* c_d, uint8_t* out_d, uint32_t* f_d) {
    hipLaunchKernelGGL(k_smul_uniform<T>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, in_d, n, k, c_d + 32, out_d, f_d);
  }));
  OG_REQUIRE(!(flags & 1), who + ": a point coordinate of the key is not below the base-field modulus");
  OG_REQUIRE(!(flags & 2), who + ": a point of the key is not on its curve");
  return OG_OK;
}

static int pk_contribute(og_ctx* ctx, const uint8_t* pkb, size_t pk_len, const uint8_t* vkb, size_t vk_len, const uint8_t dd[32], std::vector<uint8_t>& pk,
                  std::vector<uint8_t>& vk) {
  const std::string who = "og_pk_contribute";
  const Fr dv = zfr_load(dd);
  OG_REQUIRE(fe_lt_modulus(dv) && !dv.is_zero(), who + ": the contribution must be canonical (below the group order) and non-zero");
  PkView pv;
  VkView vv;
  OG_TRY(pk_view(pkb, pk_len, who, &pv));  // (the matrices ride along unread: no CSR check)
  OG_REQUIRE(pv.flags <= 1 && pv.word9 == 0, who + ": bad key header");
  OG_TRY(vk_view(vkb, vk_len, who, &vv));
  OG_REQUIRE(vk_is_of_pk(vv, pv), who + ": the verifying key does not belong to this proving key (n_pub, alpha, beta or delta differ)");
  const size_t nl = pv.nl, nh = pv.nh, l_off = pv.off(pv.query[3]), h_off = pv.off(pv.query[4]);
  K256 kd, kinv;
  memcpy(kd.l, dd, 32);
  uint8_t inv_b[32];
  zfr_store(inv_b, fe_from_mont(fe_inv(fe_to_mont(dv))));
  memcpy(kinv.l, inv_b, 32);

  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev dev;
  pk.assign(pkb, pkb + pk_len);
  vk.assign(vkb, vkb + vk_len);
  std::vector<uint8_t> lh((nl + nh) * 64), lh_out((nl + nh) * 64);  // the L and H queries behind each other: one launch
  memcpy(lh.data(), pkb + l_off, nl * 64);
  memcpy(lh.data() + nl * 64, pkb + h_off, nh * 64);
  OG_TRY(smul_uniform<Fq>(ctx, dev, lh.data(), nl + nh, kinv, lh_out.data(), who));
  memcpy(&pk[l_off], lh_out.data(), nl * 64);
  memcpy(&pk[h_off], lh_out.data() + nl * 64, nh * 64);
  OG_TRY(smul_uniform<Fq>(ctx, dev, pv.delta1, 1, kd, &pk[PK_DELTA1], who));
  OG_TRY(smul_uniform<Fq2>(ctx, dev, pv.delta2, 1, kd, &pk[PK_DELTA2], who));
  memcpy(&vk[VK_DELTA2], &pk[PK_DELTA2], 128);
  return OG_OK;
}

// ---- the two checks ---------------------------------------------------------------------------------------------------------
// og_ptau_verify: every section of the file is a geometric sequence with the ratio tauG2[1] carries (`snarkjs powersoftau
// verify` without the contribution transcripts); og_pk_verify: a key is og_setup_ptau's key for this circuit and this file up
// to its delta (`snarkjs zkey verify`, likewise).  Both are linear in the points: per section one vector of challenge scalars
// rho, ONE digit sort of it, and an msm_run per sum over plain bases -- the section from point 0 and from point 1, or a key's
// query and the rebuilt key's -- then one two-pairing product per check on the host.  The library draws no randomness: the
// scalars are Fiat-Shamir, MiMC7 of a seed that is the Keccak-256 of every input byte and of the (section, index) pair,
// truncated to 128 bits; a section that is not what it should be satisfies one linear relation in uniformly drawn rho, which
// happens with probability about 2^-128.  Every check runs; the verdict is a bit mask.
static const char* const PTAU_CHECK[5] = {"tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"};
static const char* const PK_CHECK[6] = {"header", "queries", "ic", "delta", "L", "H"};

static std::string failed_names(uint32_t mask, const char* const* names, int n) {
  std::string out;
  for (int k = 0; k < n; k++)
    if (mask & (1u << k)) out += (out.empty() ? "" : ", ") + std::string(names[k]);
  return out;
}

// seed = keccak256(tag | keccak256(part) ...) mod r, canonical
static void challenge_seed(const char* tag, std::initializer_list<std::pair<const uint8_t*, size_t>> parts, uint8_t seed[32]) {
  std::vector<uint8_t> pre(tag, tag + strlen(tag));
  uint8_t h[32];
  for (const auto& p : parts) {
    keccak256(p.first, p.second, h);
    pre.insert(pre.end(), h, h + 32);
  }
  keccak256(pre.data(), pre.size(), h);
  zfr_store(seed, fe_from_mont(fe_to_mont(zfr_load(h))));  // (any 256-bit value goes in, its residue comes out)
}

static bool any_infinity(const uint8_t* pts, size_t n, size_t pb) {
  for (size_t i = 0; i < n; i++)
    if (all_zero(pts + i * pb, pb)) return true;
  return false;
}

// f <- f * (the Miller value of e(+-p, q)); canonical affine bytes of points on their curves, q in the subgroup.  A point at
// infinity pairs to one.  false: the loop met a vertical line, which points of order r never give.
static bool miller_factor(const uint8_t* p64, const uint8_t* q128, bool neg, Fq12& f) {
  if (all_zero(p64, 64) || all_zero(q128, 128)) return true;
  G1A p = {fe_to_mont(ld_any<FqParams>(p64)), fe_to_mont(ld_any<FqParams>(p64 + 32))};
  if (neg) p.y = fe_neg(p.y);
  const G2A q = {fq2_from_bytes(q128), fq2_from_bytes(q128 + 64)};
  Fq12 m;
  if (!miller_loop(p, q, m)) return false;
  f = f12_mul(f, m);
  return true;
}
// e(a1, b1) == e(a2, b2): one product of two Miller values, the second with its G1 side negated, one final exponentiation
static bool pairing_eq(const uint8_t* a1, const uint8_t* b1, const uint8_t* a2, const uint8_t* b2) {
  Fq12 f = f12_one();
  if (!miller_factor(a1, b1, false, f) || !miller_factor(a2, b2, true, f)) return false;
  return f12_is_one(final_exponentiation(f));
}

// out[k] = sum over i < n of rho_i . bases_d[k][i], k < nb: canonical affine bytes on the host.  rho = the challenge scalars
// of (seed, section); every sum takes the SAME vector through the SAME digit sort.  bases_d[k]: n affine Montgomery points of
// one group on the device, used where they lie -- plain bases, no window tables for sums that run once.
static int challenge_sums(og_ctx* ctx, const uint8_t* seed_d, uint32_t section, bool g2, size_t n, const uint8_t* const* bases_d, int nb, uint8_t* out) {
  const size_t pb = g2 ? 128 : 64;
  memset(out, 0, (size_t)nb * pb);
  if (n == 0) return OG_OK;
  ZDev dev;
  uint8_t *rho_d, *res_d, *aff_d;
  OG_TRY(dev.get(n * 32, &rho_d));
  OG_TRY(dev.get((size_t)nb * 2 * pb, &res_d));
  OG_TRY(dev.get((size_t)nb * pb, &aff_d));
  hipLaunchKernelGGL(k_challenge_scalars, dim3(grid_for(n, 128)), dim3(128), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, seed_d, section, n, rho_d);
  OG_HIP(hipGetLastError());
  const int c = (int)msm_pick_c(n);
  DigitSort ds;
  OG_TRY(msm_digit_sort(ctx, 0, rho_d, n * 32, n, nullptr, 1, c, 0, &ds));
  for (int k = 0; k < nb; k++) {
    og_bases b;
    b.is_g2 = g2 ? 1 : 0; b.n = n; b.c = c; b.nwin = msm_nwin(c); b.precomp = 0; b.device = ctx->device;
    b.tab_d = const_cast<uint8_t*>(bases_d[k]);
    OG_TRY(msm_run(ctx, &b, ds, res_d + (size_t)k * 2 * pb));
  }
  OG_TRY(xyzz_to_affine_bytes(ctx, g2 ? 1 : 0, res_d, aff_d, (size_t)nb));
  OG_HIP(hipMemcpyAsync(out, aff_d, (size_t)nb * pb, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

static int ctx_is_idle(og_ctx* ctx, const std::string& who) {
  // (the sums' scratch -- the digit sort, the bucket sets -- is also the scratch of a submitted prove call)
  OG_REQUIRE(ctx->jobs[0] == nullptr && ctx->jobs[1] == nullptr, who + ": a submitted prove call has not been waited for (og_job_wait) -- its scratch is in use");
  return OG_OK;
}

static int ptau_verify(og_ctx* ctx, const uint8_t* data, size_t len, uint32_t* failed_out) {
  const std::string who = "og_ptau_verify";
  BinFile bf;
  PtauHeader hd;
  OG_TRY(ptau_parse(data, len, who, &bf, &hd));
  OG_TRY(ptau_sections(bf, hd, who));
  uint8_t seed[32];
  challenge_seed("owshen_gpu og_ptau_verify 1", {{data, len}}, seed);

  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_TRY(ctx_is_idle(ctx, who));
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev keep;
  uint8_t* seed_d;
  OG_TRY(keep.get(32, &seed_d));
  OG_HIP(hipMemcpyAsync(seed_d, seed, 32, hipMemcpyHostToDevice, ctx->stream));
  const size_t np = (size_t)1 << hd.power;
  // a section at a time (its decoded copies go back before the next one comes): tauG2 first, whose second point is the ratio
  // three other checks are made against
  const struct { int id; bool g2; size_t n; } secs[4] = {{3, true, np}, {2, false, 2 * np - 1}, {4, false, np}, {5, false, np}};
  uint8_t sums[6][2][128] = {}, second[6][128] = {}, beta1_0[64], beta2[128];
  bool has_inf[7] = {};
  for (const auto& sc : secs) {
    const size_t pb = sc.g2 ? 128 : 64;
    ZDev dev;
    std::vector<uint8_t> canon;
    uint8_t* mont_d;
    OG_TRY(ptau_decode(ctx, dev, bf, sc.id, sc.g2, sc.n, sc.n, canon, &mont_d, who));
    if (sc.id == 2) OG_REQUIRE(memcmp(canon.data(), G1_GEN_BYTES, 64) == 0, who + ": " + PTAU_SEC[2] + ": the first point is not the G1 generator");
    if (sc.id == 3) {
      OG_REQUIRE(memcmp(canon.data(), G2_GEN_BYTES, 128) == 0, who + ": " + PTAU_SEC[3] + ": the first point is not the G2 generator");
      OG_TRY(g2_subgroup_check(ctx, dev, mont_d, sc.n, who + ": " + PTAU_SEC[3]));
    }
    has_inf[sc.id] = any_infinity(canon.data(), sc.n, pb);
    if (sc.n > 1) memcpy(second[sc.id], canon.data() + pb, pb);
    if (sc.id == 5) memcpy(beta1_0, canon.data(), 64);
    const uint8_t* bases[2] = {mont_d, mont_d + pb};  // S0 over points 0 .. n - 2, S1 over points 1 .. n - 1
    OG_TRY(challenge_sums(ctx, seed_d, (uint32_t)sc.id, sc.g2, sc.n - 1, bases, 2, &sums[sc.id][0][0]));
    if (!sc.g2) memcpy(sums[sc.id][1], &sums[sc.id][0][64], 64);  // (challenge_sums packs its results: G1 points are 64 B apart)
  }
  {
    ZDev dev;
    std::vector<uint8_t> canon;
    uint8_t* mont_d;
    OG_TRY(ptau_decode(ctx, dev, bf, 6, true, 1, 1, canon, &mont_d, who));
    OG_TRY(g2_subgroup_check(ctx, dev, mont_d, 1, who + ": " + PTAU_SEC[6]));
    memcpy(beta2, canon.data(), 128);
  }
  uint32_t mask = 0;
  const uint8_t* tau2_1 = second[3];
  for (int id : {2, 4, 5})  // e(S1, G2) = e(S0, tau G2)
    if (has_inf[id] || !pairing_eq(sums[id][1], G2_GEN_BYTES, sums[id][0], tau2_1)) mask |= id == 2 ? 1u : id == 4 ? 4u : 8u;
  if (has_inf[3] || !pairing_eq(second[2], sums[3][0], G1_GEN_BYTES, sums[3][1])) mask |= 2u;  // e(tau G1, S0) = e(G1, S1)
  if (all_zero(beta2, 128) || all_zero(beta1_0, 64) || !pairing_eq(beta1_0, G2_GEN_BYTES, G1_GEN_BYTES, beta2)) mask |= 16u;
  *failed_out = mask;
  if (mask) set_error(who + ": failed checks: " + failed_names(mask, PTAU_CHECK, 5));
  return OG_OK;
}

// n canonical affine points on the host -> affine Montgomery on the device; *flags: 1 a coordinate >= q, 2 a point off the curve
template <class T>
static int canon_to_mont(og_ctx* ctx, ZDev& dev, const uint8_t* in, size_t n, uint8_t** mont_d, uint32_t* flags) {
  OG_TRY(dev.get(n * Affine<T>::BYTES, mont_d));
  return lem_run(ctx, dev, Affine<T>::BYTES == 128, false, in, n, nullptr, *mont_d, flags, [&](uint8_t* in_d, uint8_t* c_d, uint8_t* out_d, uint32_t* f_d) {
    hipLaunchKernelGGL(k_canon_to_mont<T>, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in_d, n, c_d + 32, out_d, f_d);
  });
}

int points_on_curve(og_ctx* ctx, int is_g2, const uint8_t* points, size_t n, uint32_t* flags) {
  ZDev dev;
  uint8_t* mont_d = nullptr;
  return is_g2 ? canon_to_mont<Fq2>(ctx, dev, points, n, &mont_d, flags) : canon_to_mont<Fq>(ctx, dev, points, n, &mont_d, flags);
}

static int pk_verify(og_ctx* ctx, const og_r1cs* r, const uint8_t* data, size_t len, const uint8_t* pkb, size_t pk_len, const uint8_t* vkb, size_t vk_len,
              uint32_t* failed_out) {
  const std::string who = "og_pk_verify";
  OG_REQUIRE(pk_is_blob(pkb, pk_len), who + ": not an OWPK0001 blob");
  OG_REQUIRE(vk_is_blob(vkb, vk_len), who + ": not an OWVK0001 blob");
  OG_REQUIRE(rd64(pkb + PK_FLAGS) == 0, who + ": the key carries header flag " + std::to_string(rd64(pkb + PK_FLAGS)) +
                                            " (imported without its .r1cs: no C matrix) -- import it beside its .r1cs (og_zkey_import with r1cs) and verify that key");
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_TRY(ctx_is_idle(ctx, who));
  }
  std::vector<uint8_t> pk0, vk0;  // the delta = 1 key of this circuit and this file
  OG_TRY(ptau_setup(ctx, r, data, len, pk0, vk0, who));
  uint8_t seed[32];
  challenge_seed("owshen_gpu og_pk_verify 1", {{data, len}, {pkb, pk_len}, {vkb, vk_len}}, seed);
  PkView pv, pv0;
  OG_REQUIRE(pk_view(pk0.data(), pk0.size(), who, &pv0) == OG_OK, who + ": internal: the rebuilt key does not parse");
  // any other fault in the structure of the CALLER's key is a verdict, not an error (its message is replaced below)
  if (pk_view(pkb, pk_len, who, &pv) != OG_OK || pv.m != pv0.m || pv.l != pv0.l || pv.log_d != pv0.log_d || memcmp(pv.nnz, pv0.nnz, sizeof pv.nnz) != 0 ||
      vk_len != vk0.size()) {
    *failed_out = 63u;  // another shape: no query of this key is the size of the circuit's, nothing else has anything to be compared with
    set_error(who + ": failed checks: " + failed_names(63u, PK_CHECK, 6) + " (the key's header or length is not this circuit's: nothing else can be compared)");
    return OG_OK;
  }
  const size_t nl = pv0.nl, nh = pv0.nh;
  uint32_t mask = 0;
  // the matrices row for row; a key that went through a .zkey counts its rows up to the domain: the rows it adds must be empty
  bool mats = pv.n_rows >= pv0.n_rows;
  for (int k = 0; k < 3 && mats; k++) {
    mats = memcmp(pv.ptr[k], pv0.ptr[k], (pv0.n_rows + 1) * 4) == 0 && memcmp(pv.col[k], pv0.col[k], pv0.nnz[k] * 4) == 0 &&
           memcmp(pv.val[k], pv0.val[k], pv0.nnz[k] * 32) == 0;
    for (size_t i = pv0.n_rows + 1; i <= pv.n_rows && mats; i++) mats = rd32(pv.ptr[k] + i * 4) == pv0.nnz[k];
  }
  if (!mats || pv.word9 != 0 || memcmp(pv.alpha1, pv0.alpha1, 128) != 0 || memcmp(pv.beta2, pv0.beta2, 128) != 0 || memcmp(vkb, vk0.data(), VK_DELTA2) != 0)
    mask |= 1u;  // (alpha1 | beta1 in one comparison; the verifying key up to its delta2)
  if (memcmp(pv.query[0], pv0.query[0], pv0.off(pv0.query[3]) - pv0.off(pv0.query[0])) != 0) mask |= 2u;
  if (memcmp(vkb + VK_IC, &vk0[VK_IC], vk_len - VK_IC) != 0) mask |= 4u;

  std::lock_guard<std::mutex> lk(ctx->mu);
  OG_TRY(ctx_is_idle(ctx, who));
  OG_HIP(hipSetDevice(ctx->device));
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  ZDev keep;
  uint8_t* seed_d;
  OG_TRY(keep.get(32, &seed_d));
  OG_HIP(hipMemcpyAsync(seed_d, seed, 32, hipMemcpyHostToDevice, ctx->stream));
  // ---- delta
  const uint8_t *d1 = pv.delta1, *d2 = pv.delta2;
  bool d1_ok = !all_zero(d1, 64), d2_ok = !all_zero(d2, 128);
  {
    ZDev dev;
    uint8_t *d1_m, *d2_m;
    uint32_t f1 = 0, f2 = 0;
    OG_TRY(canon_to_mont<Fq>(ctx, dev, d1, 1, &d1_m, &f1));
    OG_TRY(canon_to_mont<Fq2>(ctx, dev, d2, 1, &d2_m, &f2));
    d1_ok = d1_ok && f1 == 0;
    d2_ok = d2_ok && f2 == 0;
    if (d2_ok) {
      bool outside = false;
      OG_TRY(g2_subgroup_flags(ctx, dev, d2_m, 1, &outside));
      d2_ok = !outside;
    }
  }
  if (!d1_ok || !d2_ok || memcmp(d2, vkb + VK_DELTA2, 128) != 0 || !pairing_eq(d1, G2_GEN_BYTES, G1_GEN_BYTES, d2)) mask |= 8u;
  if (!d2_ok) mask |= 16u | 32u;  // nothing to check L and H against
  // ---- L and H: e(sum rho_i Q_i, delta2) = e(sum rho_i Q0_i, G2), Q0 the delta = 1 key's query
  const struct { const uint8_t *q, *q0; size_t n; uint32_t bit; } qs[2] = {{pv.query[3], pv0.query[3], nl, 16u}, {pv.query[4], pv0.query[4], nh, 32u}};
  for (const auto& q : qs) {
    if (!d2_ok || q.n == 0) continue;
    ZDev dev;
    uint8_t *q_m, *q0_m;
    uint32_t f = 0, f0 = 0;
    OG_TRY(canon_to_mont<Fq>(ctx, dev, q.q, q.n, &q_m, &f));
    OG_TRY(canon_to_mont<Fq>(ctx, dev, q.q0, q.n, &q0_m, &f0));
    OG_REQUIRE(f0 == 0, who + ": internal: the rebuilt key holds a point off the curve");
    if (f) {  // an entry that is not canonical or not on the curve
      mask |= q.bit;
      continue;
    }
    const uint8_t* bases[2] = {q_m, q0_m};
    uint8_t s[2][64];
    OG_TRY(challenge_sums(ctx, seed_d, q.bit, false, q.n, bases, 2, &s[0][0]));
    if (!pairing_eq(s[0], d2, s[1], G2_GEN_BYTES)) mask |= q.bit;
  }
  *failed_out = mask;
  if (mask) set_error(who + ": failed checks: " + failed_names(mask, PK_CHECK, 6));
  return OG_OK;
}

}  // namespace og

using namespace og;

static int two_blobs_out(const std::vector<uint8_t>& pk, const std::vector<uint8_t>& vk, uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out, size_t* vk_len,
                         const char* who) {
  uint8_t *a = nullptr, *b = nullptr;
  size_t al = 0, bl = 0;
  OG_TRY(blob_out(pk, &a, &al, who));
  if (blob_out(vk, &b, &bl, who) != OG_OK) {
    free(a);
    return OG_ERR_INVALID;
  }
  *pk_out = a; *pk_len = al;
  *vk_out = b; *vk_len = bl;
  return OG_OK;
}

extern "C" {

int og_ptau_info(const uint8_t* ptau, size_t len, uint64_t info[4]) {
  return guarded([&]() -> int {
    OG_REQUIRE(ptau && info, "og_ptau_info: null argument");
    BinFile bf;
    PtauHeader hd;
    OG_TRY(ptau_parse(ptau, len, "og_ptau_info", &bf, &hd));
    info[0] = hd.power;
    info[1] = hd.ceremony_power;
    info[2] = bf.sec.count(2) ? bf.sec[2].second / 64 : 0;
    info[3] = bf.sec.count(12) && bf.sec.count(13) && bf.sec.count(14) && bf.sec.count(15) ? 1 : 0;
    return OG_OK;
  });
}

int og_setup_ptau(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t* ptau, size_t len, uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out,
                  size_t* vk_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && r1cs && ptau && pk_out && pk_len && vk_out && vk_len, "og_setup_ptau: null argument");
    *pk_out = *vk_out = nullptr;
    *pk_len = *vk_len = 0;
    std::vector<uint8_t> pk, vk;
    OG_TRY(ptau_setup(ctx, r1cs, ptau, len, pk, vk));
    return two_blobs_out(pk, vk, pk_out, pk_len, vk_out, vk_len, "og_setup_ptau");
  });
}

int og_pk_contribute(og_ctx* ctx, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t d[32], uint8_t** pk_out,
                     size_t* pk_out_len, uint8_t** vk_out, size_t* vk_out_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && pk && vk && d && pk_out && pk_out_len && vk_out && vk_out_len, "og_pk_contribute: null argument");
    *pk_out = *vk_out = nullptr;
    *pk_out_len = *vk_out_len = 0;
    std::vector<uint8_t> npk, nvk;
    OG_TRY(pk_contribute(ctx, pk, pk_len, vk, vk_len, d, npk, nvk));
    return two_blobs_out(npk, nvk, pk_out, pk_out_len, vk_out, vk_out_len, "og_pk_contribute");
  });
}

int og_ptau_verify(og_ctx* ctx, const uint8_t* ptau, size_t len, uint32_t* failed_out) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && ptau && failed_out, "og_ptau_verify: null argument");
    *failed_out = 0;
    return ptau_verify(ctx, ptau, len, failed_out);
  });
}

int og_pk_verify(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t* ptau, size_t len, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len,
                 uint32_t* failed_out) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && r1cs && ptau && pk && vk && failed_out, "og_pk_verify: null argument");
    *failed_out = 0;
    return pk_verify(ctx, r1cs, ptau, len, pk, pk_len, vk, vk_len, failed_out);
  });
}

}  // extern "C"
