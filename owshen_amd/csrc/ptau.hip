// Groth16 key generation from a powers-of-tau file: `snarkjs groth16 setup` on the GPU (og_setup_ptau), the one-scalar delta
// step of phase 2 (og_pk_contribute), and a host-only look at a .ptau's header (og_ptau_info).
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
//     bit), then a segmented sum in levels of at most SEG terms per lane: wire 0 of the withdraw circuit holds tens of thousands
//     of terms, and no lane ever walks more than SEG of them.
//   * H query: tau^j Z(tau) G1 = tau^(j+d) G1 - tau^j G1 at delta = 1: one subtraction per entry, no transform.
//
// The result is og_setup(r1cs, tau, alpha, beta, gamma = 1, delta = 1) byte for byte (canonical affine output does not depend
// on the path taken), which is what the tests pin; og_pk_contribute(d') then gives og_setup(.., 1, d').
//
// The file format is written down from snarkjs' published sources (powersoftau_new.js / binfileutils); no file made by snarkjs
// itself was available to test against.  Whether the file is a VALID ceremony (the geometric-sequence
// pairing checks) is `snarkjs powersoftau verify`'s job and is not checked here; what is checked on every point that is used:
// coordinates < q, on the curve, tauG1[0] / tauG2[0] the generators, G2 points in the order-r subgroup.
#include "ctx.h"
#include "field.hip.h"
#include "ec.hip.h"
#include "snarkfile.hip.h"
#include "keygen.h"
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

// terms[e] = val[e] . lag[idx[e]] (XYZZ); lag affine Montgomery, val canonical.  m1 = r - 1.
template <class T>
__global__ void __launch_bounds__(64) k_spmv_terms(const uint8_t* __restrict__ lag, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ val,
                                                  size_t nnz, K256 m1, uint8_t* __restrict__ terms) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  XYZZ<T> p = XYZZ<T>::from_affine(Affine<T>::load(lag + (size_t)idx[e] * Affine<T>::BYTES));
  const K256 k = k256_load(val + e * 32);
  uint32_t hi = 0, dm = 0;
  int top = -1;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    if (w) hi |= k.l[w];
    dm |= k.l[w] ^ m1.l[w];
    if (k.l[w]) top = 32 * w + 31 - __clz((int)k.l[w]);
  }
  if (dm == 0)
    p = xyzz_neg(p);
  else if (!(hi == 0 && k.l[0] == 1))
    p = ecntt_smul(p, k, top);  // every set bit, 255 included: [k]P = [k mod r]P, as og_setup reduces such a value (k = 0: no bit, infinity)
  p.store(terms + e * XYZZ<T>::BYTES);
}

// out[c] = sum of in[ptr[c] .. ptr[c + 1]) (an empty range: the point at infinity).  affine = 0: XYZZ out (another level
// follows); 1: canonical affine bytes (a query).
template <class T>
__global__ void __launch_bounds__(64) k_seg_sum(const uint8_t* __restrict__ in, const uint32_t* __restrict__ ptr, size_t n, uint8_t* __restrict__ out,
                                               int affine) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const uint32_t b = ptr[c], e = ptr[c + 1];
  XYZZ<T> acc = XYZZ<T>::inf();
#pragma unroll 1
  for (uint32_t i = b; i < e; i++) acc = xyzz_add(acc, XYZZ<T>::load(in + (size_t)i * XYZZ<T>::BYTES));
  if (!affine) {
    acc.store(out + c * XYZZ<T>::BYTES);
    return;
  }
  Affine<T> a = xyzz_to_affine(acc);
  a.x = FieldIO<T>::from_mont(a.x);
  a.y = FieldIO<T>::from_mont(a.y);
  a.store(out + c * Affine<T>::BYTES);
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

// ---- the file -----------------------------------------------------------------------------------------------------------------
static const uint32_t FR_WORDS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static K256 fr_order(uint32_t minus) {
  K256 k;
  memcpy(k.l, FR_WORDS, 32);
  k.l[0] -= minus;  // (the low word is 0xf0000001: no borrow for minus <= 1)
  return k;
}

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

static int g2_subgroup_check(og_ctx* ctx, ZDev& dev, const uint8_t* mont_d, size_t n, const std::string& who_sec) {
  uint8_t* f_d;
  OG_TRY(dev.get(4, &f_d));
  OG_HIP(hipMemsetAsync(f_d, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_g2_subgroup, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, mont_d, n, fr_order(0), (uint32_t*)f_d);
  OG_HIP(hipGetLastError());
  uint32_t flags = 0;
  OG_HIP(hipMemcpyAsync(&flags, f_d, 4, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  OG_REQUIRE(flags == 0, who_sec + ": a point is not in the order-r subgroup");
  return OG_OK;
}

constexpr uint32_t SEG = 32;  // terms one lane sums per level

// out_d[i] = sum over e in [tptr[i], tptr[i + 1]) of tval[e] . lag_d[tidx[e]], i < m: canonical affine, on the device
template <class T>
static int point_spmv(og_ctx* ctx, const uint8_t* lag_d, const std::vector<uint32_t>& tptr, const std::vector<uint32_t>& tidx,
                      const std::vector<uint8_t>& tval, size_t m, uint8_t* out_d) {
  const size_t nnz = tidx.size();
  ZDev dev;  // this product's scratch (terms, every level) goes back when it is done: the call's peak is its largest step
  uint8_t *idx_d, *val_d, *cur_d;
  OG_TRY(dev.get(nnz * 4, &idx_d));
  OG_TRY(dev.get(nnz * 32, &val_d));
  OG_TRY(dev.get(nnz * XYZZ<T>::BYTES, &cur_d));
  if (nnz) {
    OG_HIP(hipMemcpyAsync(idx_d, tidx.data(), nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(val_d, tval.data(), nnz * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_spmv_terms<T>, dim3(grid_for(nnz, 64)), dim3(64), 0, ctx->stream, lag_d, (const uint32_t*)idx_d, val_d, nnz, fr_order(1), cur_d);
    OG_HIP(hipGetLastError());
  }
  // levels: while some wire still holds more than SEG items, every run of SEG items of a wire becomes one
  std::vector<std::vector<uint32_t>> keep;  // the host arrays outlive their copies
  std::vector<uint32_t> cp = tptr;
  for (;;) {
    uint32_t longest = 0;
    for (size_t i = 0; i < m; i++) longest = std::max(longest, cp[i + 1] - cp[i]);
    if (longest <= SEG) break;
    std::vector<uint32_t> chunk, next(m + 1, 0);
    for (size_t i = 0; i < m; i++) {
      for (uint32_t s = cp[i]; s < cp[i + 1]; s += SEG) chunk.push_back(s);
      next[i + 1] = (uint32_t)chunk.size();
    }
    const size_t n_chunks = chunk.size();
    chunk.push_back(cp[m]);  // the wires tile the items, so chunk c ends where chunk c + 1 starts -- in its own wire or at the next one
    uint8_t *p_d, *nxt_d;
    OG_TRY(dev.get((n_chunks + 1) * 4, &p_d));
    OG_TRY(dev.get(n_chunks * XYZZ<T>::BYTES, &nxt_d));
    keep.push_back(std::move(chunk));
    OG_HIP(hipMemcpyAsync(p_d, keep.back().data(), (n_chunks + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_seg_sum<T>, dim3(grid_for(n_chunks, 64)), dim3(64), 0, ctx->stream, cur_d, (const uint32_t*)p_d, n_chunks, nxt_d, 0);
    OG_HIP(hipGetLastError());
    cur_d = nxt_d;
    cp.swap(next);
  }
  uint8_t* p_d;
  OG_TRY(dev.get((m + 1) * 4, &p_d));
  OG_HIP(hipMemcpyAsync(p_d, cp.data(), (m + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_seg_sum<T>, dim3(grid_for(m, 64)), dim3(64), 0, ctx->stream, cur_d, (const uint32_t*)p_d, m, out_d, 1);
  OG_HIP(hipGetLastError());
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

int ptau_setup(og_ctx* ctx, const og_r1cs* r, const uint8_t* data, size_t len, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk) {
  const std::string who = "og_setup_ptau";
  BinFile bf;
  PtauHeader hd;
  OG_TRY(ptau_parse(data, len, who, &bf, &hd));
  const uint64_t np = 1ull << hd.power;
  const uint64_t want[7] = {0, 0, (2 * np - 1) * 64, np * 128, np * 64, np * 64, 128};
  for (uint32_t id = 2; id <= 6; id++) {
    OG_REQUIRE(bf.sec.count(id), who + ": " + PTAU_SEC[id] + " missing");
    OG_REQUIRE(bf.sec[id].second == want[id], who + ": " + PTAU_SEC[id] + " has " + std::to_string(bf.sec[id].second) + " bytes, power " +
                                                  std::to_string(hd.power) + " asks for " + std::to_string(want[id]));
  }
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
  constexpr size_t pb = Affine<T>::BYTES;
  uint8_t *in_d, *out_d, *c_d, *f_d;
  OG_TRY(dev.get(n * pb, &in_d));
  OG_TRY(dev.get(n * pb, &out_d));
  OG_TRY(dev.get(96, &c_d));
  OG_TRY(dev.get(4, &f_d));
  alignas(16) uint8_t consts[96];
  lem_consts(pb == 128, false, consts);
  OG_HIP(hipMemcpyAsync(in_d, in, n * pb, hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemcpyAsync(c_d, consts, 96, hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemsetAsync(f_d, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_smul_uniform<T>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, in_d, n, k, c_d + 32, out_d, (uint32_t*)f_d);
  OG_HIP(hipGetLastError());
  uint32_t flags = 0;
  OG_HIP(hipMemcpyAsync(out, out_d, n * pb, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(&flags, f_d, 4, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  OG_REQUIRE(!(flags & 1), who + ": a point coordinate of the key is not below the base-field modulus");
  OG_REQUIRE(!(flags & 2), who + ": a point of the key is not on its curve");
  return OG_OK;
}

int pk_contribute(og_ctx* ctx, const uint8_t* pkb, size_t pk_len, const uint8_t* vkb, size_t vk_len, const uint8_t dd[32], std::vector<uint8_t>& pk,
                  std::vector<uint8_t>& vk) {
  const std::string who = "og_pk_contribute";
  const Fr dv = zfr_load(dd);
  OG_REQUIRE(fe_lt_modulus(dv) && !dv.is_zero(), who + ": the contribution must be canonical (below the group order) and non-zero");
  OG_REQUIRE(pk_len >= 80 + 512 && rd64(pkb) == 0x313030304b50574full, who + ": not an OWPK0001 blob");
  uint64_t hd[10];
  memcpy(hd, pkb, 80);
  const uint64_t m = hd[1], l = hd[2], power = hd[3], n_rows = hd[4];
  OG_REQUIRE(power >= 1 && power <= 28 && m >= 1 && l < m && m < (1ull << 31) && hd[8] <= 1 && hd[9] == 0, who + ": bad key header");
  const uint64_t d = 1ull << power, nl = m - l - 1, nh = d - 1;
  OG_REQUIRE(n_rows <= d, who + ": more rows than the domain holds");
  OG_REQUIRE(vk_len == 16 + 64 + 3 * 128 + (l + 1) * 64 && memcmp(vkb, "OWVK0001", 8) == 0 && rd64(vkb + 8) == l,
             who + ": the verifying key does not belong to this proving key");
  OG_REQUIRE(memcmp(vkb + 16, pkb + 80, 64) == 0 && memcmp(vkb + 16 + 64, pkb + 80 + 256, 128) == 0 && memcmp(vkb + 16 + 64 + 256, pkb + 80 + 384, 128) == 0,
             who + ": the verifying key's alpha / beta / delta differ from the proving key's");
  size_t off = 80 + 512;
  for (int k = 0; k < 3; k++) {
    OG_REQUIRE(hd[5 + k] < (1ull << 32), who + ": nnz too large");
    off += zpad32((n_rows + 1) * 4) + zpad32(hd[5 + k] * 4) + zpad32(hd[5 + k] * 32);
    OG_REQUIRE(off <= pk_len, who + ": truncated key");
  }
  off += 2 * zpad32(m * 64) + zpad32(m * 128);
  const size_t l_off = off, h_off = off + zpad32(nl * 64);
  OG_REQUIRE(h_off + zpad32(nh * 64) == pk_len, who + ": key length does not match its header");
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
  OG_TRY(smul_uniform<Fq>(ctx, dev, pkb + 80 + 128, 1, kd, &pk[80 + 128], who));    // delta1
  OG_TRY(smul_uniform<Fq2>(ctx, dev, pkb + 80 + 384, 1, kd, &pk[80 + 384], who));   // delta2
  memcpy(&vk[16 + 64 + 256], &pk[80 + 384], 128);
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

}  // extern "C"
