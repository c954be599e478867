// Groth16 prover for BN254 on gfx950: proving-key residency, batched proving.
//
// No reference counterpart.  The entry points are shaped for the reference's
// withdraw seam: `withdraw_handler` (/root/reference/src/services/api_services/withdraw.rs:27-71)
// would call og_prove between the ECDSA recover (:34) and the sequencer re-sign (:56).
//
// A call is cut into sub-batches (make_plan) and every sub-batch is issued by ONE of three schedules (prove_enqueue and the
// issue_* functions in front of it): the stage pipeline -- prep: witness, sparse products, digit sorts; math: quotient, bucket
// accumulation; tail: reduction, assembly; scratch per slot, so the memory-bound stages of sub-batch k + 1 run under the
// VALU-bound ones of k --, a call that fits one sub-batch with its queries fanned out over the streams, or sub-batches one
// after the other on a stream.  Per sub-batch, in HBM:
//   k_withdraw_*     (og_withdraw_prove_batch_d only) the sub-batch's witnesses
//   k_spmv x3        a = A z, b = B z, c = C z over the QAP rows              (CSR, one lane per row)
//   h_poly_device    3 iNTT + 3 coset NTT + pointwise + coset iNTT            (ntt.hip)
//                    A key in the evaluation form (og_pk::h_form, "the second rule") stops at the coset: iNTT + coset NTT of A z and
//                    of B z and their product -- its H tables hold the DFT of the H query, its L tables carry C z
//   msm_digit_sort   signed 16-bit digits of z, counting-sorted once per DENSITY MAP: the A query, the B query
//                    (its G1 and G2 copies share the sort) and the L query each keep only the wires whose
//                    base is not the point at infinity (bellman's "query density")
//                    A key loaded with its row-basis extension (og_pk_load_rows, key_blob.h) may run the A and / or the B query
//                    over the QAP ROWS instead -- sum_j (A z)_j [L_j(tau)], the same group element: then that query's scalars
//                    are the canonical copy of A z / B z that k_spmv leaves, sorted over the row map (og_pk::row, "the rule")
//   msm_run x4       bucket accumulate + reduce over the compacted, precomputed window tables
//   msm_digit_sort + msm_run   the H query over the quotient coefficients
//   k_assemble_*     r/s blinding (s delta2 from a fixed-base table), final sums, affine conversion, 256 B proofs
// (r, s) are explicit inputs: proofs are reproducible and bit-comparable with the oracle.
#include "ctx.h"
#include "statements.h"
#include "msm.hip.h"
#include "prover.h"
#include "field.hip.h"
#include "glv.h"
#include "ec.hip.h"
#include "key_blob.h"
#include "keygen.h"          // csr_transpose
#include "point_spmv.hip.h"  // the DFT over points and the sparse product over points: the H query's evaluation form (h_form_derive)
#include <string.h>
#include <algorithm>
#include <iterator>
#include <atomic>
#include <mutex>
#include <thread>

struct og_pk {
  uint64_t m = 0, n_pub = 0, log_d = 0, n_rows = 0;
  size_t d = 0;
  uint64_t nnz[3] = {0, 0, 0};
  uint32_t* ptr[3] = {nullptr, nullptr, nullptr};
  uint32_t* col[3] = {nullptr, nullptr, nullptr};
  uint8_t* val[3] = {nullptr, nullptr, nullptr};  // Fr, Montgomery form
  uint32_t* long_rows[3] = {nullptr, nullptr, nullptr};  // rows with more than SPMV_LONG entries (a workgroup each)
  uint32_t n_long[3] = {0, 0, 0};
  og_bases *a = nullptr, *b1 = nullptr, *b2 = nullptr, *l = nullptr, *h = nullptr;
  // density compaction: query q holds only its non-infinity bases; map[q][k] = wire of compact base k.
  // q: 0 = A, 1 = B (shared by the G1 and G2 copies), 2 = L
  uint32_t* map[3] = {nullptr, nullptr, nullptr};
  size_t n_dense[3] = {0, 0, 0};  // entries of the compact wire list (what the digit sort and the table hold)
  size_t n_real[3] = {0, 0, 0};   // ... of which bases that are not the point at infinity (og_pk_density)
  int sort_src[3] = {0, 1, 2};    // sort_src[q] = p < q: query q's wire list is query p's, and it reuses p's digit sort
  // Row form (pk_load_impl, "the rule"): query q in {0 A, 1 B} runs over the QAP rows, sum_j (M z)_j [L_j(tau)], instead of the
  // wires.  Then a / b1 (b2) ALIAS lag1 (lag2), the tables over the Lagrange points of the rows in `rmap` -- the rows with an
  // entry in a matrix that runs in row form; a row that one of two such matrices lacks has (M z)_j = 0 there, no digit, and is
  // never accumulated -- and map[q] aliases rmap.  The wire-form tables of such a query are not built.
  bool row[3] = {false, false, false};
  og_bases *lag1 = nullptr, *lag2 = nullptr;
  uint32_t* rmap = nullptr;
  size_t n_rowpts = 0;           // entries of rmap
  size_t rows_q[2] = {0, 0};     // rows with an entry in A | B
  int c_wire[3] = {0, 0, 0};     // window bits of the wire-form tables of A, B, L (og_pk_windows), built or not
  bool merge_lh = false;          // the L and H queries share one bucket set per proof (same window bits): C = sum z L + sum h H is ONE MSM
  // Evaluation form of the quotient (pk_load_impl, h_form_pays): the H tables hold E'_p = zinv / d sum_k w^(-p k) g^(-k) H_k, d
  // points in coset order, and the H query's scalars are the coset values (A z)(B z) -- no transform of C z, no inverse transform;
  // the L tables hold L_i + G'_i, G'_i = -zinv sum_j C_ji F_j the fold of C z, over the L wires and every other wire of C
  bool h_form = false;
  bool c_is_ab = false;           // header flag 1 (an imported snarkjs key, zkey.hip): no C matrix, C z := (A z) o (B z) on the domain
  uint8_t* consts1 = nullptr;  // alpha1 | beta1 | delta1, affine Montgomery (3 x 64 B)
  uint8_t* consts2 = nullptr;  // beta2 | delta2, affine Montgomery (2 x 128 B)
  uint8_t* fb_delta2 = nullptr;  // fixed-base table of delta2: 64 windows x 16 digits x 128 B
  int device = 0;
  // host copies for the proof assembly on the host (og_set_host_chains): the constants and delta2's table as they sit on the
  // device, and delta1's fixed-base table (64 x 16 XYZZ points, built on first use)
  uint8_t consts1_h[192] = {}, consts2_h[256] = {};
  std::vector<uint8_t> fb_delta2_h;
  mutable std::vector<uint8_t> fb_delta1_h;
  mutable std::once_flag fb_delta1_once;
};

namespace og {

// ---- sparse matrix x witness ---------------------------------------------------------
// out[g][row] = sum_k val[k] * x[g][col[k]] for row < n_rows, 0 for n_rows <= row < n_out.
// val_mont: values are in Montgomery form (product of a Montgomery value and a canonical x is
// canonical); out_mont: convert the row sum to Montgomery form before storing.  canon (optional): the sums of the rows < n_rows
// once more, canonical, at canon[g][row] (canon_stride per g) -- the scalars of a query that runs over the rows (og_pk::row): the
// digit sort wants canonical scalars, and the quotient destroys `out`.
__global__ void __launch_bounds__(256) k_spmv(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ col,
                                             const uint8_t* __restrict__ val, size_t n_rows, size_t n_out,
                                             const uint8_t* __restrict__ x, size_t x_stride, uint8_t* __restrict__ out,
                                             size_t out_stride, int val_mont, int out_mont, uint32_t long_row,
                                             uint8_t* __restrict__ canon, size_t canon_stride) {
  OG_FILLER_PRIO();
  size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_out) return;
  const int g = blockIdx.y;
  const uint8_t* xg = x + (size_t)g * x_stride;
  Fr acc = Fr::zero();
  if (row < n_rows) {
    if (ptr[row + 1] - ptr[row] > long_row) return;  // a workgroup takes this row (k_spmv_long)
    for (uint32_t k = ptr[row]; k < ptr[row + 1]; k++) {
      Fr v = fe_load<FrParams>(val + (size_t)k * 32);
      if (!val_mont) v = fe_to_mont(v);
      acc = fe_add(acc, fe_mul(v, fe_load<FrParams>(xg + (size_t)col[k] * 32)));
    }
    if (canon) fe_store(canon + (size_t)g * canon_stride + row * 32, fe_canon(acc));
    acc = out_mont ? fe_to_mont(acc) : fe_canon(acc);
  }
  fe_store(out + (size_t)g * out_stride + row * 32, acc);
}

// rows with more than SPMV_LONG entries (e.g. the density rows: one entry per wire): one workgroup per (row, proof),
// strided partial sums, LDS tree
constexpr uint32_t SPMV_LONG = 2048;
__global__ void __launch_bounds__(256) k_spmv_long(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ ptr,
                                                  const uint32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                  const uint8_t* __restrict__ x, size_t x_stride, uint8_t* __restrict__ out,
                                                  size_t out_stride, int val_mont, int out_mont, uint8_t* __restrict__ canon,
                                                  size_t canon_stride) {
  OG_FILLER_PRIO();
  __shared__ __align__(16) uint32_t part[256 * 8];
  const uint32_t row = rows[blockIdx.x];
  const int g = blockIdx.y;
  const uint8_t* xg = x + (size_t)g * x_stride;
  Fr acc = Fr::zero();
  for (uint32_t k = ptr[row] + threadIdx.x; k < ptr[row + 1]; k += 256) {
    Fr v = fe_load<FrParams>(val + (size_t)k * 32);
    if (!val_mont) v = fe_to_mont(v);
    acc = fe_add(acc, fe_mul(v, fe_load<FrParams>(xg + (size_t)col[k] * 32)));
  }
  fe_store(&part[threadIdx.x * 8], acc);
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d)
      fe_store(&part[threadIdx.x * 8], fe_add(fe_load<FrParams>(&part[threadIdx.x * 8]), fe_load<FrParams>(&part[(threadIdx.x + d) * 8])));
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc = fe_load<FrParams>(&part[0]);
    if (canon) fe_store(canon + (size_t)g * canon_stride + (size_t)row * 32, fe_canon(acc));
    fe_store(out + (size_t)g * out_stride + (size_t)row * 32, out_mont ? fe_to_mont(acc) : fe_canon(acc));
  }
}

__global__ void __launch_bounds__(256) k_fr_to_mont(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe_store(out + i * 32, fe_to_mont(fe_load<FrParams>(in + i * 32)));
}

// c = a o b, row by row (Montgomery form): the C z of a key without a C matrix (og_pk::c_is_ab)
__global__ void __launch_bounds__(256) k_mul_rows(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ c, size_t d) {
  OG_FILLER_PRIO();
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= d) return;
  const size_t o = ((size_t)blockIdx.y * d + row) * 32;
  fe_store(c + o, fe_mul(fe_load<FrParams>(a + o), fe_load<FrParams>(b + o)));
}

// Exact satisfiability check on the QAP row products (Montgomery form): flags[g] |= 1 if some row has a_i b_i != c_i,
// or if wire 0 of the witness is not the constant 1 (the input-consistency rows cannot see that).
__global__ void __launch_bounds__(256) k_check_rows(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const uint8_t* __restrict__ c,
                                                   size_t n_rows, size_t d, const uint8_t* __restrict__ z, size_t z_stride,
                                                   uint32_t* __restrict__ flags) {
  OG_FILLER_PRIO();
  size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (row >= n_rows) return;
  const size_t o = ((size_t)g * d + row) * 32;
  bool bad = !fe_sub(fe_mul(fe_load<FrParams>(a + o), fe_load<FrParams>(b + o)), fe_load<FrParams>(c + o)).is_zero();
  if (row == 0) {
    Fr z0 = fe_load<FrParams>(z + (size_t)g * z_stride);
    z0.l[0] ^= 1u;  // canonical 1 -> all-zero limbs
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) nz |= z0.l[i];
    bad = bad || nz != 0;
  }
  if (bad) atomicOr(&flags[g], 1u);
}

// Boundary check of caller-supplied witnesses: every wire must be the canonical encoding of an Fr element (< r).  A value
// >= r would be reduced silently by the Montgomery entry -- the proof would be one for a DIFFERENT byte string than the caller
// holds.  bad[g] = lowest offending wire of witness g (atomicMin; initialised to 0xffffffff by the caller).
__global__ void __launch_bounds__(256) k_check_canonical(const uint8_t* __restrict__ x, size_t stride, size_t count, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int g = blockIdx.y;
  if (!fe_lt_modulus(fe_load<FrParams>(x + (size_t)g * stride + i * 32))) atomicMin(&bad[g], (uint32_t)i);
}

// Lagrange basis of the size-2^log_d domain at tau: out[k] = Z(tau)/d * w^k / (tau - w^k), canonical.  At tau = w^j the formula
// is 0/0 for k = j (and fe_inv(0) = 0): that element is 1, the others are 0 through Z(tau) = 0 -- the unit vector e_j
__global__ void __launch_bounds__(256) k_lagrange(const uint8_t* __restrict__ consts, const uint8_t* __restrict__ tau_c, int log_d,
                                                 uint8_t* __restrict__ out) {
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t d = (size_t)1 << log_d;
  if (k >= d) return;
  Fr tau = fe_to_mont(fe_load<FrParams>(tau_c));
  Fr zt = tau;
  for (int i = 0; i < log_d; i++) zt = fe_sqr(zt);
  zt = fe_sub(zt, Fr::one());
  Fr b = fe_load<FrParams>(consts + 0 * 32), wk = Fr::one();
  for (size_t e = k; e; e >>= 1) {
    if (e & 1) wk = fe_mul(wk, b);
    b = fe_sqr(b);
  }
  Fr num = fe_mul(fe_mul(zt, fe_load<FrParams>(consts + 4 * 32)), wk);
  Fr den = fe_sub(tau, wk);
  fe_store(out + k * 32, fe_from_mont(den.is_zero() ? Fr::one() : fe_mul(num, fe_inv(den))));
}

int spmv_canonical(og_ctx* ctx, const uint32_t* ptr_d, const uint32_t* col_d, const uint8_t* val_d, size_t n_rows,
                   const uint8_t* x_d, uint8_t* out_d) {
  if (n_rows == 0) return OG_OK;
  hipLaunchKernelGGL(k_spmv, dim3(grid_for(n_rows, 256), 1), dim3(256), 0, ctx->stream, ptr_d, col_d, val_d, n_rows, n_rows, x_d,
                     (size_t)0, out_d, (size_t)0, 0, 0, 0xffffffffu, (uint8_t*)nullptr, (size_t)0);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int lagrange_evals(og_ctx* ctx, int log_d, const uint8_t tau[32], uint8_t* out_d) {
  uint8_t* consts = nullptr;
  OG_TRY(ntt_domain_consts(ctx, log_d, &consts));
  uint8_t* tau_d = nullptr;
  OG_TRY(arena_get(ctx, "g16.tau", 32, (void**)&tau_d));
  OG_HIP(hipMemcpyAsync(tau_d, tau, 32, hipMemcpyHostToDevice, ctx->stream));
  const size_t d = (size_t)1 << log_d;
  hipLaunchKernelGGL(k_lagrange, dim3(grid_for(d, 256)), dim3(256), 0, ctx->stream, consts, tau_d, log_d, out_d);
  OG_HIP(hipGetLastError());
  OG_HIP(hipStreamSynchronize(ctx->stream));  // tau_d / the caller's tau are released after this
  return OG_OK;
}

int scalar_mul_fixed(og_ctx* ctx, int is_g2, const uint8_t* base_host, const uint8_t* scalars_d, size_t n, uint8_t* out_d) {
  const size_t pb = is_g2 ? 128 : 64;
  const int g = is_g2 ? 1 : 0;
  uint8_t *raw = nullptr, *mont = nullptr;
  OG_TRY(arena_get(ctx, "g16.base.raw", 128, (void**)&raw));
  OG_TRY(arena_get(ctx, "g16.base.mont", 128, (void**)&mont));
  if (!ctx->fb_tab[g]) {  // fixed-base table (ecmul_impl.hip.h), kept for the life of the context
    OG_HIP(hipMalloc((void**)&ctx->fb_tab[g], 64 * 16 * pb));
    ctx->owned.push_back(ctx->fb_tab[g]);
  }
  uint8_t* tab = ctx->fb_tab[g];
  if (!ctx->fb_valid[g] || memcmp(ctx->fb_base[g], base_host, pb) != 0) {
    ctx->fb_valid[g] = false;
    OG_HIP(hipMemcpyAsync(raw, base_host, pb, hipMemcpyHostToDevice, ctx->stream));
    OG_TRY(is_g2 ? import_points_g2(ctx, raw, mont, 1) : import_points_g1(ctx, raw, mont, 1));
    OG_TRY(is_g2 ? fixed_table_g2(ctx, mont, tab) : fixed_table_g1(ctx, mont, tab));
    OG_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(ctx->fb_base[g], base_host, pb);
    ctx->fb_valid[g] = true;
  }
  OG_TRY(is_g2 ? scalar_mul_fixed_g2(ctx, tab, scalars_d, n, out_d) : scalar_mul_fixed_g1(ctx, tab, scalars_d, n, out_d));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

// ---- proving key -----------------------------------------------------------------------
// The serialized key: key_blob.h.
void pk_destroy(og_pk* pk) {
  if (!pk) return;
  (void)hipSetDevice(pk->device);
  (void)hipDeviceSynchronize();  // a submitted call (og_withdraw_prove_batch_submit_d) may still be reading the key on any stream
  for (int k = 0; k < 3; k++) {
    if (pk->ptr[k]) (void)hipFree(pk->ptr[k]);
    if (pk->col[k]) (void)hipFree(pk->col[k]);
    if (pk->val[k]) (void)hipFree(pk->val[k]);
    if (pk->long_rows[k]) (void)hipFree(pk->long_rows[k]);
  }
  for (og_bases* q : {pk->a, pk->b1, pk->b2})
    if (q != pk->lag1 && q != pk->lag2) bases_destroy(q);  // (a query in row form aliases the Lagrange tables)
  bases_destroy(pk->lag1); bases_destroy(pk->lag2); bases_destroy(pk->l); bases_destroy(pk->h);
  for (int k = 0; k < 3; k++)
    if (pk->map[k] && pk->map[k] != pk->rmap) (void)hipFree(pk->map[k]);
  if (pk->rmap) (void)hipFree(pk->rmap);
  if (pk->consts1) (void)hipFree(pk->consts1);
  if (pk->consts2) (void)hipFree(pk->consts2);
  if (pk->fb_delta2) (void)hipFree(pk->fb_delta2);
  delete pk;
}

// The rule: a query runs over the rows when rows_q x windows(rows_q) <= 0.8 x wires_q x windows(wires_q) -- additions against
// additions.  The 0.8 keeps near-ties on the wires: the wire form shares one digit sort of z with the L query (sort_src) and a
// wire that holds 0 or 1 costs it none or one addition, a row sum is a full-width scalar in every window.
bool row_form_pays(size_t rows_q, size_t wires_q) {
  if (rows_q == 0 || wires_q == 0) return false;
  const double row_adds = (double)rows_q * msm_nwin((int)msm_pick_query_c(rows_q));
  const double wire_adds = (double)wires_q * msm_nwin((int)msm_pick_query_c(wires_q));
  return row_adds <= 0.8 * wire_adds;
}

// Row form against wire form on the key's own points, once per load: for a pseudo-random vector rho (from the extension's digest;
// the identity sum_i rho_i [m_i(tau)] = sum_j (M rho)_j [L_j(tau)] holds for EVERY rho) the query over the Lagrange tables
// must give the point the blob's own query gives -- for each query that will run in row form, in each of its groups.  An
// extension made for other points (a flipped bit that stays on the curve, another tau) fails here.
static int rows_check(og_ctx* ctx, const og_pk* pk, const PkView& v, const RowsView& rv, uint8_t* stage, const std::string& who) {
  const size_t m = pk->m, nr = pk->n_rows;
  std::vector<uint8_t> rho(m * 32);
  uint64_t x = rd64(rv.digest) ^ rd64(rv.digest + 8) ^ rd64(rv.digest + 16) ^ rd64(rv.digest + 24);
  for (size_t i = 0; i < m * 4; i++) {  // splitmix64; the top word keeps 60 bits: < 2^252 < r, canonical
    x += 0x9e3779b97f4a7c15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    if ((i & 3) == 3) z &= (1ull << 60) - 1;
    memcpy(&rho[i * 8], &z, 8);
  }
  uint8_t *rho_d, *ev_d, *res_d, *aff_d;
  OG_TRY(arena_get(ctx, "g16.chk.rho", m * 32, (void**)&rho_d));
  OG_TRY(arena_get(ctx, "g16.chk.ev", nr * 32, (void**)&ev_d));
  OG_TRY(arena_get(ctx, "g16.chk.res", 512, (void**)&res_d));
  OG_TRY(arena_get(ctx, "g16.chk.aff", 256, (void**)&aff_d));
  OG_HIP(hipMemcpyAsync(rho_d, rho.data(), m * 32, hipMemcpyHostToDevice, ctx->stream));
  const int cw = (int)msm_pick_c(m);
  struct Pair { int q, src, is_g2; const char* name; };
  const Pair pairs[3] = {{0, 0, 0, "A"}, {1, 1, 0, "B (G1)"}, {1, 2, 1, "B (G2)"}};
  for (const Pair& p : pairs) {
    if (!pk->row[p.q]) continue;
    const size_t pb = p.is_g2 ? 128 : 64;
    hipLaunchKernelGGL(k_spmv, dim3(grid_for(nr, 256), 1), dim3(256), 0, ctx->stream, pk->ptr[p.q], pk->col[p.q], pk->val[p.q], nr, nr, rho_d,
                       (size_t)0, ev_d, (size_t)0, 1, 0, SPMV_LONG, (uint8_t*)nullptr, (size_t)0);
    OG_HIP(hipGetLastError());
    if (pk->n_long[p.q]) {
      hipLaunchKernelGGL(k_spmv_long, dim3(pk->n_long[p.q], 1), dim3(256), 0, ctx->stream, pk->long_rows[p.q], pk->ptr[p.q], pk->col[p.q],
                         pk->val[p.q], rho_d, (size_t)0, ev_d, (size_t)0, 1, 0, (uint8_t*)nullptr, (size_t)0);
      OG_HIP(hipGetLastError());
    }
    // the blob's query over every wire, as plain bases (a wire without a base is all zeros: infinity, skipped)
    OG_HIP(hipMemcpyAsync(stage, v.query[p.src], m * pb, hipMemcpyHostToDevice, ctx->stream));
    og_bases* wb = nullptr;
    OG_TRY(bases_create(ctx, p.is_g2, stage, m, cw, 0, &wb));
    struct Drop { og_bases* b; ~Drop() { bases_destroy(b); } } drop{wb};
    DigitSort dw, dr;
    OG_TRY(msm_digit_sort(ctx, 0, rho_d, m * 32, m, nullptr, 1, cw, 0, &dw));
    OG_TRY(msm_run(ctx, wb, dw, res_d));
    const og_bases* lag = p.is_g2 ? pk->lag2 : pk->lag1;
    OG_TRY(msm_digit_sort(ctx, 1, ev_d, nr * 32, pk->n_rowpts, pk->rmap, 1, lag->c, 1, &dr));
    OG_TRY(msm_run(ctx, lag, dr, res_d + 256));
    OG_TRY(xyzz_to_affine_bytes(ctx, p.is_g2, res_d, aff_d, 1));
    OG_TRY(xyzz_to_affine_bytes(ctx, p.is_g2, res_d + 256, aff_d + 128, 1));
    uint8_t got[256];
    OG_HIP(hipMemcpyAsync(got, aff_d, 256, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));  // (also: wb is idle before it is dropped)
    OG_REQUIRE(memcmp(got, got + 128, pb) == 0,
               who + ": row-basis extension: its points do not reproduce the key's " + p.name + " query (not the Lagrange basis of this key's tau)");
  }
  return OG_OK;
}

// The second rule: the quotient in the evaluation form -- two transforms each of A z and B z, none of C z, no inverse transform
// (6 tile passes of 11, ntt.hip) -- for a key that has a C matrix (a flag-1 key has none to fold) and a domain of 2^14 or more.
// Below that bound a call is latency-bound and the quotient is not what it waits for; and the recorded issue orders
// (tests/golden/issue_order, domains up to 2^12) are recordings of that regime: such keys issue what they always issued.
static bool h_form_pays(bool has_c, int log_d) { return has_c && log_d >= 14; }

// What a key in the evaluation form derives from its blob, once per load.  With H_k the H query,
// H_(d-1) := infinity, g the coset generator, zinv = 1 / (g^d - 1):
//   e[p]   = E'_p = zinv / d sum_k w^(-p k) g^(-k) H_k: sum_k h_k H_k = sum_p ((a b - c)(g w^p)) E'_p for every h of degree <= d - 2
//   F'_j   = -zinv / d sum_k w^(-j k) H_k,   G'_i = sum_j C_ji F'_j: sum_p c(g w^p) E'_p = -sum_i z_i G'_i (deg c < d: exact)
//   lg[i]  = L_i + G'_i for EVERY wire i (L_i = infinity for wire 0 and the public wires; all zeros: the wire has neither)
// The two sums each carry the x^(d-1) coefficient that has no H point; together it is h_(d-1) = 0 for a satisfied witness.
struct HFormTables {
  std::vector<uint8_t> e;   // d x 64 B, canonical affine, in coset order (what the last DIT pass writes)
  std::vector<uint8_t> lg;  // m x 64 B, canonical affine
};
static int h_form_derive(og_ctx* ctx, const og_pk* pk, const PkView& v, const std::string& who, HFormTables* out) {
  const size_t m = pk->m, d = pk->d, nl = v.nl, nh = v.nh, npub1 = pk->n_pub + 1, n_rows = pk->n_rows, nnz = pk->nnz[2];
  const int log_d = (int)pk->log_d;
  const FfRoots& f = ff_roots();
  OG_REQUIRE(f.ok, who + ": internal: the roots of unity are not what the field layer expects");
  OG_REQUIRE((uint64_t)d + nl < (1ull << 32) && (uint64_t)nnz + nl < (1ull << 32), who + ": key too large for the evaluation form");
  const Fr seven = fe_to_mont(fe_from_u32<FrParams>(7));
  Fr nn = Fr::one();  // d as a field element
  for (int i = 0; i < log_d; i++) nn = fe_dbl(nn);
  const Fr scale = fe_mul(fe_inv(fe_sub(zfr_pow2k(seven, log_d), Fr::one())), fe_inv(nn));  // zinv / d
  std::vector<uint8_t> tw, pre, post_e(32), post_f(32);
  pow_table(fe_inv(zfr_pow2k(f.w28_own, 28 - log_d)), Fr::one(), d / 2, tw);
  pow_table(fe_inv(seven), Fr::one(), d, pre);
  zfr_store(post_e.data(), fe_from_mont(scale));
  zfr_store(post_f.data(), fe_from_mont(fe_neg(scale)));
  ZDev dev;
  uint8_t *raw_d, *hm_d, *base_d, *e_d, *lg_d;
  OG_TRY(dev.get(std::max(d, nl) * 64, &raw_d));
  OG_TRY(dev.get(d * 64, &hm_d));
  OG_TRY(dev.get((d + nl) * 64, &base_d));  // F' | the L query, affine Montgomery: what the sparse product reads
  OG_TRY(dev.get(d * 64, &e_d));
  OG_TRY(dev.get(m * 64, &lg_d));
  OG_HIP(hipMemsetAsync(raw_d, 0, d * 64, ctx->stream));  // H_(d-1) := infinity
  OG_HIP(hipMemcpyAsync(raw_d, v.query[4], nh * 64, hipMemcpyHostToDevice, ctx->stream));
  OG_TRY(import_points_g1(ctx, raw_d, hm_d, d));
  OG_TRY(ecntt_run<Fq>(ctx, dev, hm_d, log_d, tw, &pre, &post_e, true, d, e_d, false));
  OG_TRY(ecntt_run<Fq>(ctx, dev, hm_d, log_d, tw, nullptr, &post_f, true, d, base_d, true));
  OG_HIP(hipStreamSynchronize(ctx->stream));  // (raw_d is read; the scalar vectors' copies are done)
  if (nl) {
    OG_HIP(hipMemcpyAsync(raw_d, v.query[3], nl * 64, hipMemcpyHostToDevice, ctx->stream));
    OG_TRY(import_points_g1(ctx, raw_d, base_d + d * 64, nl));
  }
  // C transposed: wire i's entries over F', and the wire's own L point with coefficient 1
  std::vector<uint32_t> cptr(n_rows + 1), ccol(nnz), tptr, trow, kptr(m + 1, 0), kidx;
  std::vector<uint8_t> cval(v.val[2], v.val[2] + nnz * 32), tval, kval;
  for (size_t r = 0; r <= n_rows; r++) cptr[r] = rd32(v.ptr[2] + r * 4);
  for (size_t e = 0; e < nnz; e++) ccol[e] = rd32(v.col[2] + e * 4);
  csr_transpose(cptr, ccol, cval, n_rows, m, tptr, trow, tval);
  kidx.reserve(nnz + nl);
  kval.reserve((nnz + nl) * 32);
  uint8_t one[32] = {1};
  for (size_t i = 0; i < m; i++) {
    kidx.insert(kidx.end(), trow.begin() + tptr[i], trow.begin() + tptr[i + 1]);
    kval.insert(kval.end(), tval.begin() + (size_t)tptr[i] * 32, tval.begin() + (size_t)tptr[i + 1] * 32);
    if (i >= npub1 && !all_zero(v.query[3] + (i - npub1) * 64, 64)) {
      kidx.push_back((uint32_t)(d + (i - npub1)));
      kval.insert(kval.end(), one, one + 32);
    }
    kptr[i + 1] = (uint32_t)kidx.size();
  }
  OG_TRY(point_spmv<Fq>(ctx, base_d, kptr, kidx, kval, m, lg_d));  // synchronises
  out->e.resize(d * 64);
  out->lg.resize(m * 64);
  OG_HIP(hipMemcpyAsync(out->e.data(), e_d, d * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(out->lg.data(), lg_d, m * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  // hooks builds: OG_H_FORM_CORRUPT=1 | 2 puts a wrong point into E' | into L + G' -- what h_form_check exists to refuse
  const long long corrupt = OG_HOOK_INT("OG_H_FORM_CORRUPT", 0);
  if (corrupt == 1 && d >= 2) memcpy(&out->e[64], &out->e[0], 64);
  for (size_t i = 0; i < m && corrupt == 2; i++) {  // (E'_0 in the place of the first folded point: on the curve, and wrong)
    if (all_zero(&out->lg[i * 64], 64)) continue;
    memcpy(&out->lg[i * 64], &out->e[0], 64);
    break;
  }
  return OG_OK;
}

// The derived tables against the blob's own queries, once per load, through the kernels the prover runs: a wrong DFT must fail
// the load, not every later proof.  u: a pseudo-random coefficient vector with u_(d-1) = 0; rho: a pseudo-random wire vector.
// The evaluation-form quotient (h_poly_device) runs on two hand-made proofs -- (a, b) = (the values of u on the domain, the
// constant g^d - 1) and (C rho, the constant 1): their coset products are u's coset values / zinv, and C rho's -- and
//   1  sum_p q1[p] E'_p = sum_k u_k H_k                                                          (the new H tables | the blob's H query)
//   2  sum_i rho_i (L_i + G'_i) + sum_p (q1 + q2)[p] E'_p = sum_i rho_i L_i + sum_k u_k H_k     (the C fold, on (rho, u))
static int h_form_check(og_ctx* ctx, const og_pk* pk, const PkView& v, uint8_t* stage, const std::string& who) {
  const size_t m = pk->m, d = pk->d, nl = v.nl, nh = v.nh, npub1 = pk->n_pub + 1;
  const int log_d = (int)pk->log_d;
  std::vector<uint8_t> sc((m + d) * 32);  // rho | u
  uint64_t x = rd64(v.query[4]) ^ rd64(v.query[4] + 32) ^ ((uint64_t)m << 32) ^ d;
  for (size_t i = 0; i < (m + d) * 4; i++) {  // splitmix64; the top word keeps 60 bits: < 2^252 < r, canonical
    x += 0x9e3779b97f4a7c15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    if ((i & 3) == 3) z &= (1ull << 60) - 1;
    memcpy(&sc[i * 8], &z, 8);
  }
  memset(&sc[(m + d - 1) * 32], 0, 32);  // u_(d-1) = 0
  std::vector<uint8_t> bh(2 * d * 32);    // b of the two proofs: the constants g^d - 1 and 1, Montgomery form
  const Fr zc = fe_sub(zfr_pow2k(fe_to_mont(fe_from_u32<FrParams>(7)), log_d), Fr::one());
  for (size_t i = 0; i < d; i++) {
    fe_store(&bh[i * 32], zc);
    fe_store(&bh[(d + i) * 32], Fr::one());
  }
  ZDev dev;
  uint8_t *sc_d, *ue_d, *a_d, *b_d, *h_d, *res_d;
  OG_TRY(dev.get((m + d) * 32, &sc_d));
  OG_TRY(dev.get(d * 32, &ue_d));
  OG_TRY(dev.get(2 * d * 32, &a_d));
  OG_TRY(dev.get(2 * d * 32, &b_d));
  OG_TRY(dev.get(2 * d * 32, &h_d));
  OG_TRY(dev.get(5 * 128, &res_d));  // new H (two proofs) | new L | the blob's H | the blob's L: XYZZ, all zeros = infinity
  const uint8_t *rho_d = sc_d, *u_d = sc_d + m * 32;
  OG_HIP(hipMemcpyAsync(sc_d, sc.data(), sc.size(), hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemcpyAsync(b_d, bh.data(), bh.size(), hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemsetAsync(res_d, 0, 5 * 128, ctx->stream));
  OG_TRY(ntt_canonical(ctx, u_d, ue_d, log_d, 1, 0, 0));
  hipLaunchKernelGGL(k_fr_to_mont, dim3(grid_for(d, 256)), dim3(256), 0, ctx->stream, ue_d, a_d, d);
  OG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_spmv, dim3(grid_for(d, 256), 1), dim3(256), 0, ctx->stream, pk->ptr[2], pk->col[2], pk->val[2], (size_t)pk->n_rows, d, rho_d,
                     (size_t)0, a_d + d * 32, (size_t)0, 1, 1, SPMV_LONG, (uint8_t*)nullptr, (size_t)0);
  OG_HIP(hipGetLastError());
  if (pk->n_long[2]) {
    hipLaunchKernelGGL(k_spmv_long, dim3(pk->n_long[2], 1), dim3(256), 0, ctx->stream, pk->long_rows[2], pk->ptr[2], pk->col[2], pk->val[2], rho_d,
                       (size_t)0, a_d + d * 32, (size_t)0, 1, 1, (uint8_t*)nullptr, (size_t)0);
    OG_HIP(hipGetLastError());
  }
  OG_TRY(h_poly_device(ctx, a_d, b_d, nullptr, nullptr, h_d, log_d, 2, 1));
  DigitSort ds;
  OG_TRY(msm_digit_sort(ctx, 0, h_d, d * 32, d, nullptr, 2, pk->h->c, 1, &ds));
  OG_TRY(msm_run(ctx, pk->h, ds, res_d));
  if (pk->n_dense[2]) {
    OG_TRY(msm_digit_sort(ctx, 0, rho_d, m * 32, pk->n_dense[2], pk->map[2], 1, pk->l->c, 1, &ds));
    OG_TRY(msm_run(ctx, pk->l, ds, res_d + 256));
  }
  // the blob's H and L queries as plain bases, in the blob's order
  const int cw = (int)msm_pick_c(std::max(nh, nl));
  og_bases *hb = nullptr, *lb = nullptr;
  struct Drop { og_bases*& b; ~Drop() { bases_destroy(b); } } drop_h{hb}, drop_l{lb};
  OG_HIP(hipMemcpyAsync(stage, v.query[4], nh * 64, hipMemcpyHostToDevice, ctx->stream));
  OG_TRY(bases_create(ctx, 0, stage, nh, cw, 0, &hb));
  OG_TRY(msm_digit_sort(ctx, 0, u_d, d * 32, nh, nullptr, 1, cw, 0, &ds));
  OG_TRY(msm_run(ctx, hb, ds, res_d + 384));
  if (nl) {
    OG_HIP(hipStreamSynchronize(ctx->stream));  // (stage is reused)
    OG_HIP(hipMemcpyAsync(stage, v.query[3], nl * 64, hipMemcpyHostToDevice, ctx->stream));
    OG_TRY(bases_create(ctx, 0, stage, nl, cw, 0, &lb));
    OG_TRY(msm_digit_sort(ctx, 0, rho_d + npub1 * 32, m * 32, nl, nullptr, 1, cw, 0, &ds));
    OG_TRY(msm_run(ctx, lb, ds, res_d + 512));
  }
  uint8_t res[5 * 128];
  OG_HIP(hipMemcpyAsync(res, res_d, sizeof res, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));  // (also: hb, lb are idle before they are dropped)
  const G1XYZZ h1 = G1XYZZ::load(res), h2 = G1XYZZ::load(res + 128), ln = G1XYZZ::load(res + 256), ho = G1XYZZ::load(res + 384),
               lo = G1XYZZ::load(res + 512);
  auto same = [](const G1XYZZ& p, const G1XYZZ& q) {
    const G1Affine a = xyzz_to_affine(p), b = xyzz_to_affine(q);
    return fe_canon(a.x) == fe_canon(b.x) && fe_canon(a.y) == fe_canon(b.y);
  };
  OG_REQUIRE(same(h1, ho), who + ": evaluation form: the derived H tables do not reproduce the key's H query");
  OG_REQUIRE(same(xyzz_add(xyzz_add(ln, h1), h2), xyzz_add(lo, ho)),
             who + ": evaluation form: the C fold in the derived L tables does not reproduce the key's L and H queries");
  return OG_OK;
}

static int pk_load_impl(og_ctx* ctx, const uint8_t* blob, size_t len, const uint8_t* rows, size_t rows_len, og_pk* pk) {
  const std::string who = rows ? "og_pk_load_rows" : "og_pk_load";
  PkView v;
  OG_TRY(pk_view(blob, len, who, &v));
  RowsView rv{};
  if (rows) OG_TRY(rows_view(rows, rows_len, v, who, &rv));  // (length, header, digest: before anything is allocated)
  OG_REQUIRE(v.flags <= 1 && v.word9 == 0, who + ": unknown header flags");
  OG_REQUIRE(!(v.flags & 1) || v.nnz[2] == 0, who + ": a key with the C = A o B flag carries no C matrix");
  OG_TRY(pk_csr_check(v, 3, who));  // (cheap, and a malformed key must never index out of bounds on the GPU)
  pk->m = v.m; pk->n_pub = v.l; pk->log_d = v.log_d; pk->n_rows = v.n_rows; pk->d = v.d;
  for (int k = 0; k < 3; k++) pk->nnz[k] = v.nnz[k];
  pk->c_is_ab = (v.flags & 1) != 0;
  const size_t m = pk->m, nl = v.nl, nh = v.nh;
  const uint8_t *c1 = blob + PK_CONSTS1, *c2 = blob + PK_CONSTS2;
  for (int k = 0; k < 3; k++) {
    OG_HIP(hipMalloc((void**)&pk->ptr[k], (pk->n_rows + 1) * 4));
    OG_HIP(hipMalloc((void**)&pk->col[k], pk->nnz[k] * 4 + 4));
    OG_HIP(hipMalloc((void**)&pk->val[k], pk->nnz[k] * 32 + 32));
    OG_HIP(hipMemcpyAsync(pk->ptr[k], v.ptr[k], (pk->n_rows + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(pk->col[k], v.col[k], pk->nnz[k] * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(pk->val[k], v.val[k], pk->nnz[k] * 32, hipMemcpyHostToDevice, ctx->stream));
    {
      std::vector<uint32_t> lr;
      for (size_t r = 0; r < pk->n_rows; r++)
        if (rd32(v.ptr[k] + (r + 1) * 4) - rd32(v.ptr[k] + r * 4) > SPMV_LONG) lr.push_back((uint32_t)r);
      pk->n_long[k] = (uint32_t)lr.size();
      if (!lr.empty()) {
        OG_HIP(hipMalloc((void**)&pk->long_rows[k], lr.size() * 4));
        OG_HIP(hipMemcpy(pk->long_rows[k], lr.data(), lr.size() * 4, hipMemcpyHostToDevice));
      }
    }
    if (pk->nnz[k]) {
      hipLaunchKernelGGL(k_fr_to_mont, dim3(grid_for(pk->nnz[k], 256)), dim3(256), 0, ctx->stream, pk->val[k], pk->val[k],
                         (size_t)pk->nnz[k]);
      OG_HIP(hipGetLastError());
    }
  }
  // constants -> affine Montgomery
  uint8_t* stage = nullptr;
  const size_t stage_bytes = std::max<size_t>(std::max<size_t>(std::max<size_t>(512, m * 128), pk->d * 64), rows ? pk->n_rows * 128 : 0);
  OG_HIP(hipMalloc((void**)&stage, stage_bytes));
  struct Guard { uint8_t* p; ~Guard() { if (p) (void)hipFree(p); } } guard{stage};
  OG_HIP(hipMalloc((void**)&pk->consts1, 256));
  OG_HIP(hipMalloc((void**)&pk->consts2, 256));
  OG_HIP(hipMemcpyAsync(stage, c1, 256, hipMemcpyHostToDevice, ctx->stream));
  OG_TRY(import_points_g1(ctx, stage, pk->consts1, 3));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  OG_HIP(hipMemcpyAsync(stage, c2, 256, hipMemcpyHostToDevice, ctx->stream));
  OG_TRY(import_points_g2(ctx, stage, pk->consts2, 2));
  OG_HIP(hipMalloc((void**)&pk->fb_delta2, 64 * 16 * 128));
  OG_TRY(fixed_table_g2(ctx, pk->consts2 + 128, pk->fb_delta2));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  pk->fb_delta2_h.resize(64 * 16 * 128);  // (140 KB: what a host-side assembly reads, og_set_host_chains)
  OG_HIP(hipMemcpy(pk->consts1_h, pk->consts1, 192, hipMemcpyDeviceToHost));
  OG_HIP(hipMemcpy(pk->consts2_h, pk->consts2, 256, hipMemcpyDeviceToHost));
  OG_HIP(hipMemcpy(pk->fb_delta2_h.data(), pk->fb_delta2, pk->fb_delta2_h.size(), hipMemcpyDeviceToHost));
  // queries -> compacted, precomputed window tables.  A wire whose base is the point at infinity (its
  // polynomial is zero at tau: the wire never occurs in that matrix) contributes nothing; drop it from the
  // table and from the digit sort.  B1 / B2 are the same polynomial in two groups, so they share one map.
  int ch = (int)msm_pick_query_c(nh);
  // Coefficients or coset values (h_form_pays), per key: decided here, once.  Hooks builds: OG_H_FORM=0|1 forces either form on
  // every key that has a C matrix.  Then the H tables and the L query come from h_form_derive, not from the blob as it stands.
  HFormTables hf;
  {
    const long long force = OG_HOOK_INT("OG_H_FORM", -1);
    pk->h_form = !pk->c_is_ab && pk->log_d >= 1 && force != 0 && (force == 1 || h_form_pays(true, (int)pk->log_d));
  }
  if (pk->h_form) {
    // The self-check below sorts and accumulates in the context's scratch (msm_digit_sort / msm_run / the NTT plan: the arena of
    // ctx->lane, on ctx->stream), as og_pk_load_rows' check does: refused while a submitted call may still be using it, and run
    // on lane 0 whatever lane and stream the last call left behind.  (The stream was drained above; keys outside the rule touch
    // no scratch and load as they always did.)
    OG_REQUIRE(ctx->jobs[0] == nullptr && ctx->jobs[1] == nullptr,
               who + ": a submitted prove call has not been waited for (og_job_wait) -- this key takes the evaluation form, and its load-time check uses the call's scratch");
    ctx->lane = 0;
    ctx->stream = ctx->lanes[0];
    OG_TRY(h_form_derive(ctx, pk, v, who, &hf));
  }
  std::vector<uint32_t> wire[3];
  for (size_t i = 0; i < m; i++) {
    if (!all_zero(v.query[0] + i * 64, 64)) wire[0].push_back((uint32_t)i);
    if (!all_zero(v.query[1] + i * 64, 64) || !all_zero(v.query[2] + i * 128, 128)) wire[1].push_back((uint32_t)i);
  }
  for (size_t i = 0; i < nl; i++)
    if (!all_zero(v.query[3] + i * 64, 64)) wire[2].push_back((uint32_t)(i + pk->n_pub + 1));
  // Queries whose wire lists coincide up to a few wires share ONE list -- the union; a wire a query does not have keeps its
  // zero bytes in that query's table, the point at infinity, which the accumulation skips -- and with it ONE digit sort per
  // sub-batch in the stage pipeline instead of one each.  The benchmark's dense padding: A and B hold every wire, L all but
  // the 7 public ones -> one sort instead of three (the three read and decompose the same witness).  The padding as built
  // (131 k | 117 k | 262 k wires) shares nothing; the natural statement shares A with L.
  for (int k = 0; k < 3; k++) pk->n_real[k] = wire[k].size();
  if (pk->h_form) {  // the L query carries C z: its own wires and every other wire of C -- wire 0 and the public wires among them
    wire[2].clear();
    for (size_t i = 0; i < m; i++)
      if (!all_zero(&hf.lg[i * 64], 64)) wire[2].push_back((uint32_t)i);
  }
  // Wires or rows (row_form_pays), per query: A decides alone, B once for its two groups.  Hooks builds: OG_ROW_FORM=0|1 forces
  // either form on every query the extension could serve (A/B runs).  L and H never change.
  std::vector<uint32_t> rlist;
  if (rows) {
    const long long force = OG_HOOK_INT("OG_ROW_FORM", -1);
    for (int q = 0; q < 2; q++) {
      for (size_t r = 0; r < pk->n_rows; r++) pk->rows_q[q] += rd32(v.ptr[q] + (r + 1) * 4) > rd32(v.ptr[q] + r * 4);
      pk->row[q] = pk->rows_q[q] > 0 && !wire[q].empty() && force != 0 && (force == 1 || row_form_pays(pk->rows_q[q], wire[q].size()));
    }
    for (size_t r = 0; r < pk->n_rows; r++)
      if ((pk->row[0] && rd32(v.ptr[0] + (r + 1) * 4) > rd32(v.ptr[0] + r * 4)) || (pk->row[1] && rd32(v.ptr[1] + (r + 1) * 4) > rd32(v.ptr[1] + r * 4)))
        rlist.push_back((uint32_t)r);
  }
  for (int q = 1; q < 3; q++)
    for (int p0 = 0; p0 < q; p0++) {
      if (pk->row[q] || pk->row[p0]) continue;  // a query over the rows has scalars of its own
      if (pk->sort_src[p0] != p0) continue;
      std::vector<uint32_t> u;
      std::set_union(wire[p0].begin(), wire[p0].end(), wire[q].begin(), wire[q].end(), std::back_inserter(u));
      const size_t least = std::min(wire[p0].size(), wire[q].size());
      if (u.size() - least > 64 || msm_pick_query_c(u.size()) != msm_pick_query_c(least)) continue;
      for (int k = 0; k < q; k++)
        if (pk->sort_src[k] == p0) wire[k] = u;  // (everyone already sharing p0's list moves to the union)
      wire[q] = u;
      pk->sort_src[q] = p0;
      break;
    }
  pk->n_rowpts = rlist.size();
  if (!rlist.empty()) {
    OG_HIP(hipMalloc((void**)&pk->rmap, rlist.size() * 4 + 4));
    OG_HIP(hipMemcpyAsync(pk->rmap, rlist.data(), rlist.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  for (int k = 0; k < 3; k++) {
    pk->c_wire[k] = (int)msm_pick_query_c(wire[k].size());
    if (pk->row[k]) {  // the row map; the wire list is not kept
      pk->n_dense[k] = rlist.size();
      pk->map[k] = pk->rmap;
      continue;
    }
    pk->n_dense[k] = wire[k].size();
    OG_HIP(hipMalloc((void**)&pk->map[k], wire[k].size() * 4 + 4));
    OG_HIP(hipMemcpyAsync(pk->map[k], wire[k].data(), wire[k].size() * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  OG_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<uint8_t> host(std::max<size_t>(std::max<size_t>(std::max<size_t>(1, m * 128), pk->d * 64), rlist.size() * 128));
  if (!rlist.empty()) {
    // ONE table per group over the Lagrange points of the rows in rlist: A and B1 share the G1 one.  The points are checked
    // first -- every coordinate below q, every point on its curve -- and against the key's own queries below (rows_check).
    for (int g2 = 0; g2 < (pk->row[1] ? 2 : 1); g2++) {
      const size_t pb = g2 ? 128 : 64;
      uint32_t flags = 0;
      OG_TRY(points_on_curve(ctx, g2, g2 ? rv.g2 : rv.g1, pk->n_rows, &flags));
      OG_REQUIRE(!(flags & 1), who + ": row-basis extension: a coordinate of a " + (g2 ? "G2" : "G1") + " point is not below the base-field modulus");
      OG_REQUIRE(!(flags & 2), who + ": row-basis extension: a " + (g2 ? "G2" : "G1") + " point is not on its curve");
      for (size_t k = 0; k < rlist.size(); k++) memcpy(host.data() + k * pb, (g2 ? rv.g2 : rv.g1) + (size_t)rlist[k] * pb, pb);
      OG_HIP(hipMemcpyAsync(stage, host.data(), rlist.size() * pb, hipMemcpyHostToDevice, ctx->stream));
      OG_TRY(bases_create(ctx, g2, stage, rlist.size(), (int)msm_pick_query_c(rlist.size()), 1, g2 ? &pk->lag2 : &pk->lag1));  // synchronises
    }
    if (pk->row[0]) pk->a = pk->lag1;
    if (pk->row[1]) { pk->b1 = pk->lag1; pk->b2 = pk->lag2; }
    OG_TRY(rows_check(ctx, pk, v, rv, stage, who));
  }
  struct QSpec { int src, mapk, is_g2; og_bases** dst; };
  const QSpec qs[4] = {{0, 0, 0, &pk->a}, {1, 1, 0, &pk->b1}, {2, 1, 1, &pk->b2}, {3, 2, 0, &pk->l}};
  for (const QSpec& q : qs) {
    if (pk->row[q.mapk]) continue;  // runs over the rows: no wire-form table
    const size_t pb = q.is_g2 ? 128 : 64;
    const std::vector<uint32_t>& w = wire[q.mapk];
    const bool folded = q.src == 3 && pk->h_form;  // L_i + G'_i, indexed by wire
    const uint8_t* src = folded ? hf.lg.data() : v.query[q.src];
    const size_t shift = q.src == 3 && !folded ? pk->n_pub + 1 : 0;  // l_query is indexed from wire n_pub + 1
    const size_t q_len = q.src == 3 && !folded ? nl : m;
    for (size_t k = 0; k < w.size(); k++) {
      if (w[k] >= shift && w[k] - shift < q_len) memcpy(host.data() + k * pb, src + (w[k] - shift) * pb, pb);
      else memset(host.data() + k * pb, 0, pb);  // a wire of the shared list this query has no base for: infinity
    }
    OG_HIP(hipMemcpyAsync(stage, host.data(), w.size() * pb, hipMemcpyHostToDevice, ctx->stream));
    OG_TRY(bases_create(ctx, q.is_g2, stage, w.size(), (int)msm_pick_query_c(w.size()), 1, q.dst));  // synchronises the stream
  }
  // the quotient leaves h_poly_device in bit-reversed order (ntt.hip): store the H query in that order.  Position
  // d - 1 is its own reversal, so the d - 1 bases stay the first d - 1 positions.  The evaluation form: E', d points, as derived
  // -- the coset values leave the last DIT pass in natural order.  The window bits are the coefficient form's either way.
  const size_t h_pts = pk->h_form ? pk->d : nh;
  if (pk->h_form) memcpy(host.data(), hf.e.data(), h_pts * 64);
  for (size_t k = 0; k < nh && !pk->h_form; k++) {
    size_t r = 0;
    for (uint64_t bit = 0; bit < pk->log_d; bit++) r |= ((k >> bit) & 1) << (pk->log_d - 1 - bit);
    memcpy(host.data() + k * 64, v.query[4] + r * 64, 64);
  }
  OG_HIP(hipMemcpyAsync(stage, host.data(), h_pts * 64, hipMemcpyHostToDevice, ctx->stream));
  // C = sum z_i L_i + sum h_j H_j is ONE multi-scalar multiplication: when the H query can take the L query's window size, the
  // two share a bucket set per proof (msm_run_phase) -- one bucket reduction, one heavy-bucket tail and one window combine per
  // proof instead of two, and at 17 bits the H query's 131 071 points cost 15 additions each instead of 16.  (17 bits needs
  // n x 15 < 2^23 entries for the two-level radix sort, msm.hip: n = the h_pts scalars that are sorted; the size rule nh >= 512
  // stays the key's own query, so that a key's window bits do not depend on the form.)  Hooks builds: OG_MERGE_LH=0 keeps the queries apart (A/B).
  const int cl = pk->l->c;
  const bool h_takes_cl = cl == ch || (cl == 17 && (double)h_pts * 15 < (double)(1u << 23) && nh >= 512) || (cl == 16 && nh >= 512);
  if (OG_HOOK_INT("OG_MERGE_LH", 1) && h_takes_cl && (cl == 16 || cl == 17 || cl == ch)) {
    ch = cl;
    pk->merge_lh = true;
  }
  OG_TRY(bases_create(ctx, 0, stage, h_pts, ch, 1, &pk->h));
  if (pk->h_form) OG_TRY(h_form_check(ctx, pk, v, stage, who));
  return OG_OK;
}

// out[0..3] = n_wires, n_pub, log_d, n_rows: the key's header
void pk_info(const og_pk* pk, uint64_t out[4]) {
  out[0] = pk->m; out[1] = pk->n_pub; out[2] = pk->log_d; out[3] = pk->n_rows;
}

// out[0..3] = window bits of the A, B (G1 and G2 copies), L and H queries' precomputed tables (msm_pick_query_c)
void pk_windows(const og_pk* pk, uint64_t out[4]) {
  for (int k = 0; k < 3; k++) out[k] = (uint64_t)pk->c_wire[k];  // (the blob's wire queries, also where one runs over the rows: pk_query_form)
  out[3] = pk->h->c;
}

// What each of the five queries A | B1 | B2 | L | H actually runs, four words each: form (0 over the wires, 1 over the QAP rows;
// H: 0, over the quotient's coefficients; L and H: 2, the evaluation form -- H over the coset values of (A z)(B z), L with C z
// folded in), points (the entries its digit sort visits and its table holds), window bits, table (queries with the
// same number share ONE set of window tables: A and B1 in row form)
void pk_query_form(const og_pk* pk, uint64_t out[20]) {
  const og_bases* q[5] = {pk->a, pk->b1, pk->b2, pk->l, pk->h};
  const int mapk[5] = {0, 1, 1, 2, -1};
  for (int k = 0; k < 5; k++) {
    out[4 * k + 0] = mapk[k] >= 0 && pk->row[mapk[k]] ? 1 : k >= 3 && pk->h_form ? 2 : 0;
    out[4 * k + 1] = q[k]->n;
    out[4 * k + 2] = (uint64_t)q[k]->c;
    int first = k;
    for (int j = k - 1; j >= 0; j--)
      if (q[j] == q[k]) first = j;
    out[4 * k + 3] = (uint64_t)first;
  }
}

// out[0..2] = bases kept by the A, B (G1 and G2 copies) and L queries after density compaction; out[3] = the H query's d - 1
void pk_density(const og_pk* pk, uint64_t out[4]) {
  for (int k = 0; k < 3; k++) out[k] = pk->n_real[k];
  out[3] = pk->d - 1;
}

// HBM bytes of the resident key: CSR matrices, the five queries' per-window tables, wire maps, constants
uint64_t pk_bytes(const og_pk* pk) {
  uint64_t b = 0;
  for (int k = 0; k < 3; k++)
    b += (pk->n_rows + 1) * 4 + pk->nnz[k] * 36 + 36 + (uint64_t)pk->n_long[k] * 4 + (pk->row[k] ? 0 : pk->n_dense[k] * 4 + 4);
  if (pk->rmap) b += pk->n_rowpts * 4 + 4;
  const og_bases* qs[5] = {pk->a, pk->b1, pk->b2, pk->l, pk->h};
  for (int k = 0; k < 5; k++) {
    const og_bases* q = qs[k];
    if (!q || std::find(qs, qs + k, q) != qs + k) continue;  // (a shared table -- A and B1 over the rows -- counts once)
    b += (uint64_t)(q->n ? q->n : 1) * (q->precomp ? q->nwin : 1) * (q->is_g2 ? 128 : 64);
  }
  return b + 256 + 256 + 64 * 16 * 128;
}

// rows (optional): the key's OWPR0001 row-basis extension (key_blob.h); a wrong one is refused, OG_ERR_INVALID
int pk_load(og_ctx* ctx, const uint8_t* blob, size_t len, const uint8_t* rows, size_t rows_len, og_pk** out) {
  og_pk* pk = new og_pk();
  pk->device = ctx->device;
  int r = pk_load_impl(ctx, blob, len, rows, rows_len, pk);
  if (r != OG_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    pk_destroy(pk);
    return r;
  }
  *out = pk;
  return OG_OK;
}

// ---- proving ---------------------------------------------------------------------------
// glv.h's (lambda, beta) must be a PAIR: phi(x, y) = (beta x, y) has to be multiplication by lambda -- the other primitive cube
// root of unity of Fq goes with lambda^2, and a mismatched pair would assemble valid-looking but WRONG A / C for every call of
// <= 64 proofs while every scalar decomposition still verifies.  Checked once per process with the group law of ec.hip.h on the
// host: [lambda] G == (beta x_G, y_G) for G = (1, 2).  On failure the GLV path is off (the plain 254-bit chains are used).
bool glv_pair_ok() {
  static const bool ok = [] {
    const Fq one = Fq::one();
    const Fq two = fe_add(one, one);
    const Affine<Fq> g{one, two};
    XYZZ<Fq> acc = XYZZ<Fq>::inf();
    for (int bit = 255; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((glv::LAMBDA[bit >> 6] >> (bit & 63)) & 1) acc = xyzz_madd(acc, g);
    }
    const Affine<Fq> got = xyzz_to_affine(acc);
    uint32_t bw[8];
    for (int i = 0; i < 4; i++) { bw[2 * i] = (uint32_t)glv::BETA[i]; bw[2 * i + 1] = (uint32_t)(glv::BETA[i] >> 32); }
    const Fq want_x = fe_mul(one, fe_to_mont(fe_from_words<FqParams>(bw)));  // beta * x_G, x_G = 1
    return fe_canon(got.x) == fe_canon(want_x) && fe_canon(got.y) == fe_canon(two);
  }();
  return ok;
}

static int choose_sub_batch(og_ctx* ctx, const og_pk* pk, size_t n) {
  // Large sub-batches amortise the latency-bound tails (reduction levels, scans: a few hundred microseconds each
  // whatever the batch).  Scratch per proof and per scratch slot: the digit entries of the sorts (4 B x nwin x the compacted
  // query sizes -- a shared wire list counted once -- twice: partition + final order), five d x 32 B polynomial buffers, the
  // witness, bucket sets and reduction levels; bounded to ~64 GiB per scratch slot (two slots in the stage pipeline) of
  // the 288 GB -- the 2^18-wire circuit with 17-bit windows (2^16 buckets per set) is ~230 MB per proof, and 256 proofs per
  // sub-batch still fit -- and to what the device has left: (free memory + what this context's arena already holds) x 0.85
  // over the slots, so a GPU shared with other work gets smaller sub-batches instead of a failed allocation.
  // A query in row form sorts its own scalars at its own window count (the entries of rmap), keeps a canonical copy of its row
  // sums (SubBatch::evc) and has the bucket set of ITS window bits.
  size_t pts = pk->d, row_entries = 0, evc = 0;
  const og_bases* wq[3] = {pk->a, pk->b1, pk->l};
  int c_max = pk->l->c;
  for (int q = 0; q < 3; q++) {
    if (pk->row[q]) {
      row_entries += (size_t)wq[q]->nwin * pk->n_dense[q];
      evc += pk->n_rows * 32;
      c_max = std::max(c_max, wq[q]->c);
    } else if (pk->sort_src[q] == q) {
      pts += pk->n_dense[q];
    }
  }
  const size_t entries = (size_t)pk->l->nwin * pts + row_entries;
  const size_t per = entries * 4 * 2 + pk->d * 32 * 5 + pk->m * 32 + evc + ((size_t)1 << (c_max - 1)) * (4 * 128 + 256) * 2;
  size_t budget = (size_t)64 << 30, free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) {
    size_t mine = 0;
    for (const auto& kv : ctx->arena) mine += kv.second.second;
    budget = std::min(budget, std::max<size_t>((size_t)1 << 30, (size_t)((double)(free_b + mine) * 0.85) / og_ctx::PIPE_SLOTS));
  }
  // og_set_scratch_budget: the operator's bound on what the sub-batch slots may reserve together (a GPU shared with other work)
  if (ctx->scratch_budget) budget = std::min(budget, std::max<size_t>(per, ctx->scratch_budget / og_ctx::PIPE_SLOTS));
  size_t sb = budget / (per ? per : 1);
  if (const char* e = getenv("OG_SUB_BATCH")) sb = (size_t)atoi(e);
  // At most 256 proofs per sub-batch for the 2^18-wire circuit (~230 MB of scratch per proof: two slots of 256 are 118 GB),
  // more for smaller statements -- up to 1024 where a proof needs <= 40 MB: the natural depth-32 statement (26 k wires, 38 MB per
  // proof) in sub-batches of 252 launches kernels too short to fill the chip and pays 17 latency-bound tails per 4096 proofs.
  // Same box, batch 4096 (hooks builds: OG_SUB_CAP): cap 256 -> 4 297 / 4 280 proofs/s, 512 -> 4 642 / 4 641, 1024 -> 4 817,
  // 2048 -> 4 816 (profiles/r05_ab_sub_cap.txt).
  const size_t cap_by_size = std::max<size_t>(256, std::min<size_t>(1024, ((size_t)40 << 30) / (per ? per : 1)));
  sb = std::max<size_t>(1, std::min<size_t>(sb, (size_t)OG_HOOK_INT("OG_SUB_CAP", (long long)cap_by_size)));
  return (int)std::min(sb, n);
}

// Optional in-lane witness generation (withdraw is the one statement routed here): the sub-batch's witnesses are produced by the
// lane that proves them (into lane-private scratch), so the latency-bound MiMC7 walk overlaps the other lane.
struct StatementGen {
  const Statement* st;
  StatementArgs args;
  const uint8_t* inputs_d;  // n records of record_bytes(*st, args.depth)
};

// Window-sharded PROVING (round 6; north_star: "MSM windows shard naturally across GPUs", BASELINE.json configs[3]).  A rank
// of a `world`-rank group runs the whole front of the prover on its own copy of the inputs -- witness, sparse products,
// quotient: replicated, they are latency chains or a few per cent of a proof -- but sorts and accumulates only the windows
// k = rank (mod world) of every query.  The key's tables are per window (tab[k][i] = 2^(c k) P_i: ONE bucket set per query), so
// a rank's share of a query is ONE point per proof and the shares simply add: no Horner step, no per-window slots.  The call
// leaves them in `partials_d` -- five arrays, A | B1 | L | H (n x 128 B each, XYZZ over Fq) | B2 (n x 256 B, XYZZ over Fq2),
// PARTIAL_BYTES per proof -- instead of assembling proofs; the host's all-gather (RCCL inside og_multi_*, torch.distributed in
// owshen_amd/shard.py) and prove_from_partials finish the call.  No reference line: the caller it serves is the
// one-request-per-call site /root/reference/src/services/api_services/withdraw.rs:27-71.
struct WinShard {
  int rank = 0, world = 1;
  uint8_t* partials_d = nullptr;
};
constexpr size_t PARTIAL_BYTES = 4 * 128 + 256;

// How a call of n proofs is cut into sub-batches and which of the three schedules runs them (prove_enqueue; og_prove_plan
// reports it, so that a bench line can say what the step actually was).
struct ProvePlan {
  int sb_max = 1;
  bool split = false, sym = false, pipe = false;
  std::vector<int> plan;
};

static int make_plan(og_ctx* ctx, const og_pk* pk, size_t n, ProvePlan* out) {
  const bool two_lanes = ctx->n_lanes >= 2;
  int sb_max = choose_sub_batch(ctx, pk, n);
  const size_t split_max = (size_t)OG_HOOK_INT("OG_SPLIT_MAX", 1024);  // the largest call that fans its queries out (below) instead of halving (hooks builds: OG_SPLIT_MAX=1 restores round 5)
  if (two_lanes && (size_t)sb_max * 2 > n && n >= 2 && n > split_max) sb_max = (int)((n + 1) / 2);
  // A call that is one small sub-batch (the single-withdraw case) has nothing to pipeline across sub-batches; instead the
  // B query (sort + its G1 and G2 MSMs) runs on lane 1 while lane 0 does the quotient and the A, L, H queries: at this
  // size no launch fills the chip, so the two streams genuinely run side by side.
  // Round 6: the same for EVERY call that fits one sub-batch (up to 1024 requests).  Until then such a call was cut in two halves
  // run side by side (`sym` below: each half walks its five MSMs -- five latency-bound tails -- one after the other) or, from 128
  // requests on, sent through the stage pipeline, which has nothing to overlap when there is one sub-batch or two.  Fanned out,
  // the call waits for its longest query instead of their sum.  Same box, interleaved (profiles/r06i_ab_split_max.txt), natural
  // statement: 2 requests 15.7 -> 12.2 ms, 8: 17.5 -> 14.2, 16: 20.3 -> 17.3, 64: 30.0 -> 26.4, 128: 47.7 -> 39.6, 256: 76.0 ->
  // 64.1, 512: 124 -> 116, 1024: level; with the host walking the chains 2: 5.5 -> 2.9, 8: 6.8 -> 4.8, 64: 22.2 -> 19.5;
  // 2^18-wire shape 2: 19.1 -> 15.0, 16: 39.6 -> 36.4, 64: 95.7 -> 87.6, 256: 321 -> 313.
  const bool split = two_lanes && n <= (size_t)sb_max && n <= std::max<size_t>(split_max, 1);
  // Sub-batches too small to fill the chip (a handful of requests) are latency-bound end to end: there, whole sub-batches
  // run side by side on the two streams (`sym`), which is worth ~1.5x (batch 8: 46 vs 68 ms); from 64 proofs per
  // sub-batch on, the stage pipeline (`pipe`) takes over.
  const int pipe_min = (int)OG_HOOK_INT("OG_PIPE_MIN", 64);  // test hook: reach the pipeline at toy sizes
  const bool sym = two_lanes && !split && sb_max < pipe_min;
  const bool pipe = two_lanes && !split && !sym;
  // Sub-batch plan.  A call starts cold: nothing can run on the math stream until the first sub-batch's witnesses, sparse
  // products and sorts exist, and that preparation takes as long as the sub-batch is big.  So the pipelined path RAMPS: a
  // small first sub-batch (its preparation is short, its math covers the preparation of a larger second one), then full
  // size, and the remainder is spread so that no straggler sub-batch is left at the end (1024 proofs at sb_max = 245 used
  // to end on a sub-batch of 44).  OG_SUB_PLAN="64,192,256" overrides (sizes are clamped to sb_max; the last repeats).
  std::vector<int>& plan = out->plan;
  plan.clear();
  {
    size_t left = n;
    if (const char* e = pipe ? OG_HOOK_STR("OG_SUB_PLAN") : nullptr) {
      int last = sb_max;
      for (const char* q = e; *q && left;) {
        OG_REQUIRE(atoi(q) >= 1, "OG_SUB_PLAN: every sub-batch size must be >= 1 (empty or non-numeric entry)");
        last = std::min(sb_max, atoi(q));
        plan.push_back((int)std::min<size_t>(last, left));
        left -= plan.back();
        while (*q && *q != ',') q++;
        if (*q == ',') q++;
      }
      while (left) {
        plan.push_back((int)std::min<size_t>(last, left));
        left -= plan.back();
      }
    } else if (pipe && n > (size_t)sb_max) {
      const int first = std::max(1, std::max(pipe_min, sb_max / 4));  // (OG_PIPE_MIN=0 with sb_max < 4 must not plan an empty sub-batch)
      plan.push_back(first);
      left -= first;
      const size_t parts = (left + sb_max - 1) / sb_max;
      for (size_t k = 0; k < parts; k++) {
        const size_t sz = (left + (parts - k) - 1) / (parts - k);
        plan.push_back((int)sz);
        left -= sz;
      }
    } else {
      while (left) {
        plan.push_back((int)std::min<size_t>(sb_max, left));
        left -= plan.back();
      }
    }
  }
  out->sb_max = sb_max; out->split = split; out->sym = sym; out->pipe = pipe;
  return OG_OK;
}

// sizes_out[0 .. *count_out) = the sub-batches a call of n proofs is cut into; *mode_out = 0 one stream, serial; 1 a call of <= 16 requests, its queries
// fanned out over the streams; 2 whole sub-batches side by side on two streams; 3 the stage pipeline
int prove_plan(og_ctx* ctx, const og_pk* pk, size_t n, uint32_t* sizes_out, size_t cap, size_t* count_out, int* mode_out) {
  ProvePlan pp;
  OG_TRY(make_plan(ctx, pk, n, &pp));
  if (count_out) *count_out = pp.plan.size();
  if (mode_out) *mode_out = pp.pipe ? 3 : pp.sym ? 2 : pp.split ? 1 : 0;
  for (size_t k = 0; k < pp.plan.size() && k < cap; k++) sizes_out[k] = (uint32_t)pp.plan[k];
  return OG_OK;
}

// ---- proof assembly on the HOST (og_set_host_chains) ---------------------------------------------------------------------------
// What is left of a request once its MSMs are done is five scalar multiplications and three inversions: chains of ~3 400 / ~380
// dependent field products, which a lone wave walks at 0.42 us per product (k_assemble_g1_muls_glv + finish + k_assemble_g2:
// 2.2-2.5 ms of a 3.7 ms request whose witness the host already walks) and a server core at 20-50 ns.  So in the same opt-in
// mode the five query results (640 B per proof) come down instead of the proof and the host runs the formulas of
// ecmul_impl.hip.h with the library's own group law (ec.hip.h is host code too: og_verify uses it):
//   A = alpha + Am + r delta1        B = beta2 + B2m + s delta2        C = L + H + s (alpha + Am) + r (beta1 + B1m) + (r s) delta1
// r delta1, (r s) delta1 and s delta2 through fixed-base tables (64 additions each), the other two by 4-bit windows.  The proofs
// are affine and canonical, so the bytes are the kernels'.
template <class T>
static XYZZ<T> host_mul_window4(const XYZZ<T>& p, const uint32_t k[8]) {
  XYZZ<T> tab[16];
  tab[1] = p;
  for (int d = 2; d < 16; d++) tab[d] = d == 2 ? xyzz_dbl(p) : xyzz_add(tab[d - 1], p);
  XYZZ<T> acc = XYZZ<T>::inf();
  for (int w = 63; w >= 0; w--) {
    if (w != 63) for (int e = 0; e < 4; e++) acc = xyzz_dbl(acc);
    const uint32_t dgt = (k[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (dgt) acc = xyzz_add(acc, tab[dgt]);
  }
  return acc;
}
static const std::vector<uint8_t>& host_fb_delta1(const og_pk* pk) {  // tab[w * 16 + d] = d 16^w delta1 (XYZZ; d = 0 unused)
  std::call_once(pk->fb_delta1_once, [&]() {
    pk->fb_delta1_h.resize(64 * 16 * G1XYZZ::BYTES);
    G1XYZZ pw = G1XYZZ::from_affine(G1Affine::load(pk->consts1_h + 128));
    for (int w = 0; w < 64; w++) {
      G1XYZZ q = pw;
      for (int d = 1; d < 16; d++) {
        q.store(pk->fb_delta1_h.data() + (size_t)(w * 16 + d) * G1XYZZ::BYTES);
        q = xyzz_add(q, pw);
      }
      pw = q;  // 16 * (16^w delta1)
    }
  });
  return pk->fb_delta1_h;
}
// The terms that need only (r, s) -- r delta1, (r s) delta1, beta2 + s delta2 -- are formed while the GPU still runs the call's MSMs
// (host_assemble_fixed, at the end of prove_enqueue: 128 + 128 + 256 B per proof, XYZZ); what waits for the results is the rest.
constexpr size_t HOST_FIXED_BYTES = 2 * G1XYZZ::BYTES + G2XYZZ::BYTES;
static void host_assemble_fixed(const og_pk* pk, const uint8_t* rs, uint8_t* out) {
  uint32_t r[8], s[8], p[8];
  memcpy(r, rs, 32);
  memcpy(s, rs + 32, 32);
  fe_to_words(p, fe_from_mont(fe_mul(fe_to_mont(fe_from_words<FrParams>(r)), fe_to_mont(fe_from_words<FrParams>(s)))));  // r s mod the group order
  const uint8_t* fb1 = host_fb_delta1(pk).data();
  auto fixed1 = [&](const uint32_t k[8]) {
    G1XYZZ acc = G1XYZZ::inf();
    for (int w = 0; w < 64; w++) {
      const uint32_t d = (k[w >> 3] >> ((w & 7) * 4)) & 15u;
      if (d) acc = xyzz_add(acc, G1XYZZ::load(fb1 + (size_t)(w * 16 + d) * G1XYZZ::BYTES));
    }
    return acc;
  };
  fixed1(r).store(out);
  fixed1(p).store(out + G1XYZZ::BYTES);
  G2XYZZ B = G2XYZZ::from_affine(G2Affine::load(pk->consts2_h));  // beta2 + s delta2 (k_assemble_g2's table, any order: the sum is the sum)
  for (int w = 0; w < 64; w++) {
    const uint32_t d = (s[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (d) B = xyzz_madd(B, G2Affine::load(pk->fb_delta2_h.data() + (size_t)(w * 16 + d) * G2Affine::BYTES));
  }
  B.store(out + 2 * G1XYZZ::BYTES);
}
static void host_assemble_one(const og_pk* pk, const uint8_t* rs, const uint8_t* fixed, const uint8_t* ra, const uint8_t* rb1,
                              const uint8_t* rb2, const uint8_t* rl, const uint8_t* rh, uint8_t* proof, bool helper_thread) {
  uint32_t r[8], s[8];
  memcpy(r, rs, 32);
  memcpy(s, rs + 32, 32);
  const G1Affine alpha = G1Affine::load(pk->consts1_h), beta1 = G1Affine::load(pk->consts1_h + 64);
  const G1XYZZ a_full = xyzz_madd(G1XYZZ::load(ra), alpha), b1_full = xyzz_madd(G1XYZZ::load(rb1), beta1);
  const G1XYZZ A = xyzz_add(a_full, G1XYZZ::load(fixed));
  G1XYZZ C = xyzz_add(G1XYZZ::load(rl), G1XYZZ::load(rh));
  G1XYZZ prod[2];
  auto mul = [&](size_t k) { prod[k] = k == 0 ? host_mul_window4(a_full, s) : host_mul_window4(b1_full, r); };
  if (helper_thread) host_parallel_for(2, mul);  // one request: its two variable-base products side by side (a call of several has a thread per proof already)
  else { mul(0); mul(1); }
  C = xyzz_add(xyzz_add(C, prod[0]), prod[1]);
  C = xyzz_add(C, G1XYZZ::load(fixed + G1XYZZ::BYTES));
  const G2XYZZ B = xyzz_add(G2XYZZ::load(rb2), G2XYZZ::load(fixed + 2 * G1XYZZ::BYTES));
  G1Affine a = xyzz_to_affine(A), c = xyzz_to_affine(C);
  a.x = fe_from_mont(a.x); a.y = fe_from_mont(a.y);
  c.x = fe_from_mont(c.x); c.y = fe_from_mont(c.y);
  G2Affine b = xyzz_to_affine(B);
  b.x = FieldIO<Fq2>::from_mont(b.x); b.y = FieldIO<Fq2>::from_mont(b.y);
  a.store(proof);
  b.store(proof + 64);
  c.store(proof + 192);
}
static void assemble_fixed_on_host(const og_pk* pk, const uint8_t* rs, size_t n, std::vector<uint8_t>& fixed) {
  fixed.resize(n * HOST_FIXED_BYTES);
  (void)host_fb_delta1(pk);  // (built once, before the threads)
  host_parallel_for(n, [&](size_t g) { host_assemble_fixed(pk, rs + g * 64, fixed.data() + g * HOST_FIXED_BYTES); });
}
// res: the five result arrays of the call on the host, [A n x 128 | B1 n x 128 | B2 n x 256 | L n x 128 | H n x 128]
static void assemble_on_host(const og_pk* pk, const uint8_t* rs, const uint8_t* fixed, const uint8_t* res, size_t n, uint8_t* proofs) {
  const uint8_t *ra = res, *rb1 = ra + n * 128, *rb2 = rb1 + n * 128, *rl = rb2 + n * 256, *rh = rl + n * 128;
  host_parallel_for(n, [&](size_t g) {
    host_assemble_one(pk, rs + g * 64, fixed + g * HOST_FIXED_BYTES, ra + g * 128, rb1 + g * 128, rb2 + g * 256, rl + g * 128, rh + g * 128,
                      proofs + g * 256, n == 1);
  });
}

// serial numbers of jobs (og_job::id)
static uint64_t next_job_id() {
  static std::atomic<uint64_t> n{1};
  return n.fetch_add(1);
}

// Latency-bound calls (a handful of requests) hand the assembly the GLV halves of its four scalars r, r s, s, r (glv.h): eight
// half-length chains per proof instead of four of 254 bits.  A scalar whose decomposition does not verify (never seen; a
// non-canonical r or s would do it) sends the whole call down the plain path (out stays empty).  OG_GLV=0 turns it off (A/B).
static void glv_halves(const uint8_t* rs, size_t n, std::vector<uint8_t>& out) {
  out.clear();
  const size_t glv_max = !glv_pair_ok() ? 0 : OG_HOOK_SET("OG_GLV") ? (OG_HOOK_INT("OG_GLV", 1) ? (size_t)1 << 30 : 0) : 64;  // (read per call: tests run both forms)
  if (n > glv_max) return;
  out.resize(n * 128);
  for (size_t g = 0; g < n && !out.empty(); g++) {
    const uint8_t *rb = rs + g * 64, *sb = rs + g * 64 + 32;
    uint32_t rw[8], sw[8], pw[8];
    memcpy(rw, rb, 32);
    memcpy(sw, sb, 32);
    fe_to_words(pw, fe_from_mont(fe_mul(fe_to_mont(fe_from_words<FrParams>(rw)), fe_to_mont(fe_from_words<FrParams>(sw)))));  // r s mod the group order
    uint8_t* o = out.data() + g * 128;
    if (!glv::decompose(rb, o) || !glv::decompose(reinterpret_cast<const uint8_t*>(pw), o + 32) || !glv::decompose(sb, o + 64)) out.clear();
    else memcpy(o + 96, o, 32);  // the fourth product is r (beta + B1m): r again
  }
}

// ---- the batched prover: one call, enqueued ----------------------------------------------------------------------------------
// prove_enqueue issues ALL the work of a call and returns an og_job; prove_finish waits for it and copies the results out.
//   call_begin      call-level buffers, (r, s) / GLV halves up on the copy stream, the drain rule between two calls
//   sub_front       what every sub-batch starts with, on the stream the schedule chose: witnesses, canonical check, public wires
//   sub_rows        the three sparse products and the satisfiability check;  sub_quotient: h = (A z . B z - C z) / Z
//   issue_fan_out | issue_pipeline | issue_serial     ONE of the three schedules (make_plan) takes the sub-batch from there
//                   to "its results exist", assembly included; each owns its streams and events
//   job_publish     the og_job and one completion event per stream
// The MSMs learn their stream through the context (ctx->stream, ctx->lane, tail_stream, msm_tag, after_heavy_ev,
// sort_beside_acc): every function here that sets one of them puts it back (LaneGuard on the error paths).
//
// witnesses (z_d): n x m x 32 B canonical, device (or null with `gen` / `z_host`).  rs: n x 64 B host.  proofs: n x 256 B host.
// pub_out (optional, host): n x n_pub x 32 B, the public wires 1..n_pub of every witness -- what the caller hands the verifier
// with the proof (withdraw: root, nullifier_hash, ...), so that it does not have to generate the witness a second time.
static int prove_finish(og_job* job, size_t* first_bad);

struct ProveCall {
  og_ctx* ctx;
  const og_pk* pk;
  size_t n;
  ProvePlan plan;
  int call_slot;
  const StatementGen* gen;      // the witnesses: generated per sub-batch | host memory | the caller's device buffer (canonical
  const uint8_t *z_host, *z_d;  // unless trusted_z)
  bool trusted_z;
  const WinShard* sh;  // a window-sharded front: the five results are the call's output, nothing is assembled
  bool host_asm;       // og_set_host_chains: the host assembles (prove_finish)
  const uint8_t* rs;   // host
  uint8_t *proofs, *pub_out;
  uint8_t *res[5], *rs_d, *proofs_d, *asm_tmp, *glv_d, *pub_d;  // device, per call slot; res: A | B1 | B2 | L | H, an XYZZ point per proof
  size_t asm_lanes;
  uint32_t *flags, *bad;  // [n] unsatisfied | [n] first non-canonical wire / record field
  bool assembles() const { return !sh && !host_asm; }
};
struct SubBatch {
  size_t g0;  // first proof
  int sb, slot;  // proofs; scratch namespace (ctx->lane) and, in the stage pipeline, event set
  const uint8_t* zs;
  uint8_t *ev[3], *tmp, *h;  // A z | B z | C z, quotient scratch, h
  uint8_t* evc[2];           // A z | B z over the rows < n_rows once more, canonical (sub_rows): the scalars of a query in row form
  uint8_t* res(const ProveCall& c, int k) const { return c.res[k] + g0 * (k == 2 ? 256 : 128); }
  uint8_t* asm_tmp(const ProveCall& c) const { return c.asm_tmp + g0 * c.asm_lanes * 128 * 17; }  // (its products and tables: its own region)
  const uint8_t* glv(const ProveCall& c) const { return c.glv_d ? c.glv_d + g0 * 128 : nullptr; }
};

// the digit sort of witness query q (0 A | 1 B | 2 L) over its compacted wire list into sort slot `slot`, and of h into sort
// slot 2 (d - 1 coefficients, or -- evaluation form -- d coset values); a sharded front sorts only this rank's windows k = rank (mod world)
static int sub_sort(const ProveCall& c, const SubBatch& s, int slot, int q, DigitSort* out) {
  const og_pk* pk = c.pk;
  // the scalars: the witness through the query's wire map, or -- row form -- (A z) / (B z) through the row map.  The canonical
  // copy sub_rows left, not ev[]: that one is in Montgomery form and the quotient destroys it, on another stream in two of the
  // three schedules.  So the only order a row-form sort needs is "after sub_rows", and sub_rows is on its stream or behind ev0.
  const uint8_t* scalars = q < 2 && pk->row[q] ? s.evc[q] : s.zs;
  const size_t stride = q < 2 && pk->row[q] ? (size_t)pk->n_rows * 32 : pk->m * 32;
  return msm_digit_sort_windows(c.ctx, slot, scalars, stride, pk->n_dense[q], pk->map[q], s.sb, (q == 0 ? pk->a : q == 1 ? pk->b1 : pk->l)->c,
                                1, c.sh ? c.sh->rank : 0, c.sh ? c.sh->world : 1, out);
}
static int sub_sort_h(const ProveCall& c, const SubBatch& s, DigitSort* out) {
  return msm_digit_sort_windows(c.ctx, 2, s.h, c.pk->d * 32, c.pk->h_form ? c.pk->d : c.pk->d - 1, nullptr, s.sb, c.pk->h->c, 1, c.sh ? c.sh->rank : 0,
                                c.sh ? c.sh->world : 1, out);
}

static int call_begin(ProveCall& c) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  const size_t n = c.n;
  const std::string cs = "#" + std::to_string(c.call_slot);  // call-level buffers exist once per call slot
  const char* resn[5] = {"g16.res.a", "g16.res.b1", "g16.res.b2", "g16.res.l", "g16.res.h"};
  uint8_t** res = c.res;
  if (c.sh) {  // the queries' results ARE the call's output: this rank's partial sums, array by array
    res[0] = c.sh->partials_d; res[1] = res[0] + n * 128; res[3] = res[1] + n * 128; res[4] = res[3] + n * 128; res[2] = res[4] + n * 128;
  } else {
    for (int k = 0; k < 5; k++) OG_TRY(arena_get(ctx, (resn[k] + cs).c_str(), n * (k == 2 ? 256 : 128), (void**)&res[k]));
  }
  OG_TRY(arena_get(ctx, ("g16.rs" + cs).c_str(), n * 64, (void**)&c.rs_d));
  OG_TRY(arena_get(ctx, ("g16.proofs" + cs).c_str(), n * 256, (void**)&c.proofs_d));
  // og_set_host_chains: a call of a handful of requests leaves its assembly to the host (assemble_on_host, in prove_finish)
  c.host_asm = !c.sh && ctx->host_chains_max > 0 && n <= (size_t)ctx->host_chains_max;
  std::vector<uint8_t> glv_h;
  if (c.assembles()) glv_halves(c.rs, n, glv_h);
  c.asm_lanes = glv_h.empty() ? 4 : 8;
  OG_TRY(arena_get(ctx, ("g16.asm" + cs).c_str(), n * c.asm_lanes * 128 * 17, (void**)&c.asm_tmp));  // results + window tables of 16 points per lane
  c.glv_d = nullptr;
  if (!glv_h.empty()) OG_TRY(arena_get(ctx, ("g16.glv" + cs).c_str(), n * 128, (void**)&c.glv_d));
  OG_TRY(arena_get(ctx, ("g16.flags" + cs).c_str(), n * 8, (void**)&c.flags));
  c.bad = c.flags + n;
  c.pub_d = nullptr;
  if (c.pub_out && pk->n_pub) OG_TRY(arena_get(ctx, ("g16.pub" + cs).c_str(), n * pk->n_pub * 32, (void**)&c.pub_d));
  // (r, s) go in on the copy stream, which never holds compute: the copy does not queue behind a previous call's kernels,
  // and every stream of this call may read rs_d once the host has seen it complete
  if (!c.sh) OG_HIP(hipMemcpyAsync(c.rs_d, c.rs, n * 64, hipMemcpyHostToDevice, ctx->copy_lane));  // (a sharded front assembles nothing: no blinding yet)
  if (c.glv_d) OG_HIP(hipMemcpyAsync(c.glv_d, glv_h.data(), n * 128, hipMemcpyHostToDevice, ctx->copy_lane));
  OG_HIP(hipStreamSynchronize(ctx->copy_lane));
  if (ctx->pipe_ev[0][0] == nullptr)
    for (int p = 0; p < og_ctx::PIPE_SLOTS; p++)
      for (int e = 0; e < og_ctx::PIPE_EVENTS; e++) OG_HIP(hipEventCreateWithFlags(&ctx->pipe_ev[p][e], hipEventDisableTiming));
  ctx->sort_beside_acc = c.plan.pipe;
  // A call may be enqueued while the previous one is still running (og_withdraw_prove_batch_submit_d).  Between two calls
  // of the stage pipeline the scratch slots are guarded by their events; any other combination shares scratch without such
  // guards, so the streams are drained first (a no-op for the blocking entry points, which left them idle).
  if (!(c.plan.pipe && ctx->last_call_piped)) OG_HIP(drain_streams(ctx));
  ctx->last_call_piped = c.plan.pipe;
  return OG_OK;
}

// on ctx->stream, in scratch namespace ctx->lane (the schedule set both)
static int sub_front(const ProveCall& c, SubBatch& s) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  const size_t m = pk->m, d = pk->d, g0 = s.g0, sb_max = (size_t)c.plan.sb_max;
  const char* evn[3] = {"g16.eva", "g16.evb", "g16.evc"};
  for (int k = 0; k < 3; k++) OG_TRY(arena_get(ctx, evn[k], sb_max * d * 32, (void**)&s.ev[k]));
  const char* evcn[2] = {"g16.eva.c", "g16.evb.c"};
  for (int k = 0; k < 2; k++) {
    s.evc[k] = nullptr;
    if (pk->row[k]) OG_TRY(arena_get(ctx, evcn[k], sb_max * pk->n_rows * 32, (void**)&s.evc[k]));
  }
  OG_TRY(arena_get(ctx, "g16.tmp", 32, (void**)&s.tmp));
  OG_TRY(arena_get(ctx, "g16.h", sb_max * d * 32, (void**)&s.h));
  s.zs = c.z_d ? c.z_d + g0 * m * 32 : nullptr;
  OG_HIP(hipMemsetAsync(c.bad + g0, 0xff, (size_t)s.sb * 4, ctx->stream));
  if (const StatementGen* gen = c.gen) {
    const uint8_t* records = gen->inputs_d + g0 * record_bytes(*gen->st, gen->args.depth);
    uint8_t* zbuf = nullptr;
    OG_TRY(records_check_enqueue(*gen->st, ctx, gen->args, records, (size_t)s.sb, c.bad + g0));
    OG_TRY(arena_get(ctx, "g16.zgen", sb_max * m * 32, (void**)&zbuf));
    OG_TRY(gen->st->witness(*gen->st, ctx, gen->args, records, (size_t)s.sb, zbuf));
    s.zs = zbuf;
  } else if (c.z_host) {
    // witnesses in HOST memory (og_prove_batch): the sub-batch crosses PCIe into its slot's staging buffer -- in the stage
    // pipeline on the prep stream, under the math stage of the previous sub-batch like everything else that stream does.
    // (Pageable memory: the call holds the host until the copy is done; the math work of sub-batch k is already enqueued by then.)
    uint8_t* zbuf = nullptr;
    OG_TRY(arena_get(ctx, "g16.zgen", sb_max * m * 32, (void**)&zbuf));
    OG_HIP(hipMemcpyAsync(zbuf, c.z_host + g0 * m * 32, (size_t)s.sb * m * 32, hipMemcpyHostToDevice, ctx->stream));
    s.zs = zbuf;
  }
  if (!c.gen && !c.trusted_z) {  // caller-supplied witnesses: every wire must be canonical (one more read of the witness)
    hipLaunchKernelGGL(k_check_canonical, dim3(grid_for(m, 256), s.sb), dim3(256), 0, ctx->stream, s.zs, m * 32, m, c.bad + g0);
    OG_HIP(hipGetLastError());
  }
  if (c.pub_d)  // wires 1..n_pub of each witness of the sub-batch (a strided device-to-device copy)
    OG_HIP(hipMemcpy2DAsync(c.pub_d + g0 * pk->n_pub * 32, pk->n_pub * 32, s.zs + 32, m * 32, pk->n_pub * 32, (size_t)s.sb,
                            hipMemcpyDeviceToDevice, ctx->stream));
  return OG_OK;
}

static int sub_rows(const ProveCall& c, const SubBatch& s) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  const size_t m = pk->m, d = pk->d;
  const int sb = s.sb;
  for (int k = 0; k < 3; k++) {
    ProfScope ps(ctx, PROF_SPMV, (double)pk->nnz[k] * sb);
    if (k == 2 && pk->c_is_ab) {
      hipLaunchKernelGGL(k_mul_rows, dim3(grid_for(d, 256), sb), dim3(256), 0, ctx->stream, s.ev[0], s.ev[1], s.ev[2], d);
      OG_HIP(hipGetLastError());
      continue;
    }
    uint8_t* canon = k < 2 && pk->row[k] ? s.evc[k] : nullptr;  // a query over the rows: its scalars, out of the quotient's way
    hipLaunchKernelGGL(k_spmv, dim3(grid_for(d, 256), sb), dim3(256), 0, ctx->stream, pk->ptr[k], pk->col[k], pk->val[k],
                       (size_t)pk->n_rows, d, s.zs, m * 32, s.ev[k], d * 32, 1, 1, SPMV_LONG, canon, (size_t)pk->n_rows * 32);
    OG_HIP(hipGetLastError());
    if (pk->n_long[k]) {
      hipLaunchKernelGGL(k_spmv_long, dim3(pk->n_long[k], sb), dim3(256), 0, ctx->stream, pk->long_rows[k], pk->ptr[k], pk->col[k],
                         pk->val[k], s.zs, m * 32, s.ev[k], d * 32, 1, 1, canon, (size_t)pk->n_rows * 32);
      OG_HIP(hipGetLastError());
    }
  }
  OG_HIP(hipMemsetAsync(c.flags + s.g0, 0, (size_t)sb * 4, ctx->stream));
  if (pk->n_rows) {
    hipLaunchKernelGGL(k_check_rows, dim3(grid_for(pk->n_rows, 256), sb), dim3(256), 0, ctx->stream, s.ev[0], s.ev[1], s.ev[2],
                       (size_t)pk->n_rows, d, s.zs, m * 32, c.flags + s.g0);
    OG_HIP(hipGetLastError());
  }
  OG_STEP(ctx, "g16.spmv");
  return OG_OK;
}

static int sub_quotient(const ProveCall& c, const SubBatch& s) {
  ProfScope ps(c.ctx, PROF_HPOLY, (double)c.pk->d * s.sb);
  OG_TRY(h_poly_device(c.ctx, s.ev[0], s.ev[1], s.ev[2], s.tmp, s.h, (int)c.pk->log_d, s.sb, c.pk->h_form ? 1 : 0));
  OG_STEP(c.ctx, "g16.hpoly");
  return OG_OK;
}

// The L and H queries of a sub-batch.  With pk->merge_lh (pk_load) they are ONE multi-scalar multiplication over one bucket
// set: the L half accumulates and stops -- its result slot is the point at infinity --, the H half adds to the same buckets
// and is reduced once.
static int msm_l(const ProveCall& c, const SubBatch& s, const DigitSort& ds_l) {
  if (!c.pk->merge_lh) return msm_run(c.ctx, c.pk->l, ds_l, s.res(c, 3));
  OG_HIP(hipMemsetAsync(s.res(c, 3), 0, (size_t)s.sb * 128, c.ctx->stream));
  return msm_run_phase(c.ctx, c.pk->l, ds_l, nullptr, MSM_FIRST);
}
static int msm_h(const ProveCall& c, const SubBatch& s, const DigitSort& dh) {
  return msm_run_phase(c.ctx, c.pk->h, dh, s.res(c, 4), c.pk->merge_lh ? MSM_SECOND : MSM_FULL);
}

// the sub-batch's proofs from its five results, in one part on ctx->stream (latency-bound scalar multiplications)
static int sub_assemble(const ProveCall& c, const SubBatch& s) {
  if (!c.assembles()) return OG_OK;
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  ProfScope ps_asm(ctx, PROF_ASSEMBLE, (double)s.sb);
  OG_TRY(assemble_g1(ctx, pk->consts1, c.rs_d + s.g0 * 64, s.res(c, 0), s.res(c, 1), s.res(c, 3), s.res(c, 4), (size_t)s.sb, s.asm_tmp(c),
                     c.proofs_d + s.g0 * 256, s.glv(c)));
  OG_TRY(assemble_g2(ctx, pk->consts2, pk->fb_delta2, c.rs_d + s.g0 * 64, s.res(c, 2), (size_t)s.sb, c.proofs_d + s.g0 * 256));
  OG_STEP(ctx, "g16.assemble");
  return OG_OK;
}

// ---- schedule 1: a call that fits one sub-batch fans its queries out --------------------------------------------------------
// Nothing here fills the chip, and every MSM ends in a chain of ~140 dependent additions (its bucket reduction: 0.9 ms in G1,
// 2.5 ms in G2).  So the four witness queries fan out -- B's sort and G2 MSM on stream 1, its G1 MSM (same sorted entries) on
// the copy stream, A on the tail stream, L on the aux stream -- while stream 0 goes on to the sparse products, the quotient and
// the H query; the assembly joins them.  (Round 2 ran A, L, H one after the other on stream 0.)  The side streams are issued
// BEFORE stream 0's sparse products: launch latency sits in front of every stream.  L and H stay apart here: side by side.
// The proofs are assembled in two parts (ecmul_impl.hip.h k_assemble_g1_early / _late; OG_ASM_EARLY=0: A/B, the one-part form):
// what needs A and B1 only runs on A's stream beside the quotient and the H query, C = L + H + three of the products is left.
// Events: ctx->ev0 the witness is complete, ctx->ev1 B's half of the proof, the rest ctx.h FanEvent.
static int issue_fan_out(const ProveCall& c, SubBatch& s) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  hipEvent_t* fan = ctx->pipe_ev[0];
  hipStream_t s0 = ctx->lanes[0], s_b2 = ctx->lanes[1], s_b1 = ctx->copy_lane, s_a = ctx->tail_lane, s_l = ctx->aux_lane;
  const bool asm_early = c.assembles() && OG_HOOK_INT("OG_ASM_EARLY", 1) != 0;
  const uint8_t* rs_sub = c.rs_d + s.g0 * 64;
  uint8_t* proofs_sub = c.proofs_d + s.g0 * 256;
  auto side = [&](int lane_id, hipStream_t st, hipEvent_t after) -> int {
    ctx->lane = lane_id;  // scratch namespace
    ctx->stream = st;
    OG_HIP(hipStreamWaitEvent(st, after, 0));
    return OG_OK;
  };
  ctx->lane = s.slot;
  ctx->stream = s0;
  OG_TRY(sub_front(c, s));
  // a key with a query in row form: that query's scalars are A z / B z, so the sparse products come BEFORE the fan-out and ev0
  // says "the witness and the row sums are complete" (the launch latency this puts in front of the side streams is three kernels')
  const bool rows_first = pk->row[0] || pk->row[1];
  if (rows_first) OG_TRY(sub_rows(c, s));
  OG_HIP(hipEventRecord(ctx->ev0, s0));  // the witness is complete
  DigitSort dsb, dsa, dsl, dh;
  OG_TRY(side(1, s_b2, ctx->ev0));
  OG_TRY(sub_sort(c, s, 1, 1, &dsb));
  OG_HIP(hipEventRecord(fan[FAN_B_SORTED], s_b2));
  OG_TRY(msm_run(ctx, pk->b2, dsb, s.res(c, 2)));
  {  // B's half of the proof is assembled right here, on the stream that produced B2: the G2 query is the longest chain of
     // a request (its bucket reduction: 2.5 ms), and its 1.2 ms of assembly (s delta2 from the fixed-base table, one
     // inversion) used to queue behind the G1 half on stream 0 instead of running beside it
    ProfScope ps_asm(ctx, PROF_ASSEMBLE, 0.0);  // (0 items: the G1 half below counts the sub-batch's proofs, og_profile_read must not see them twice)
    if (c.assembles())  // (a wave per proof, the sum as a tree: OG_ASM_G2_TREE=0 is the lane per proof it replaced here)
      OG_TRY(assemble_g2(ctx, pk->consts2, pk->fb_delta2, rs_sub, s.res(c, 2), (size_t)s.sb, proofs_sub, OG_HOOK_INT("OG_ASM_G2_TREE", 1) != 0));
  }
  OG_HIP(hipEventRecord(ctx->ev1, s_b2));
  OG_TRY(side(4, s_b1, fan[FAN_B_SORTED]));
  OG_TRY(msm_run(ctx, pk->b1, dsb, s.res(c, 1)));
  OG_HIP(hipEventRecord(fan[FAN_B1_DONE], s_b1));
  OG_TRY(side(2, s_a, ctx->ev0));
  OG_TRY(sub_sort(c, s, 1, 0, &dsa));
  OG_TRY(msm_run(ctx, pk->a, dsa, s.res(c, 0)));
  if (asm_early) {
    ProfScope ps_asm(ctx, PROF_ASSEMBLE, 0.0);  // (0 items: as for the G2 half above)
    OG_HIP(hipStreamWaitEvent(s_a, fan[FAN_B1_DONE], 0));
    OG_TRY(assemble_g1_early(ctx, pk->consts1, rs_sub, s.res(c, 0), s.res(c, 1), (size_t)s.sb, s.asm_tmp(c), proofs_sub, s.glv(c),
                             fan[FAN_PRODUCTS]));
  }
  OG_HIP(hipEventRecord(fan[FAN_A_DONE], s_a));
  OG_TRY(side(3, s_l, ctx->ev0));
  OG_TRY(sub_sort(c, s, 1, 2, &dsl));
  OG_TRY(msm_run(ctx, pk->l, dsl, s.res(c, 3)));
  OG_HIP(hipEventRecord(fan[FAN_L_DONE], s_l));
  ctx->lane = s.slot;
  ctx->stream = s0;
  if (!rows_first) OG_TRY(sub_rows(c, s));
  OG_TRY(sub_quotient(c, s));
  OG_TRY(sub_sort_h(c, s, &dh));
  OG_TRY(msm_run_phase(ctx, pk->h, dh, s.res(c, 4), MSM_FULL));
  OG_STEP(ctx, "g16.msm");
  if (asm_early) {  // C's sum waits for L and the four PRODUCTS; A's own sum and inversion join at the end
    OG_HIP(hipStreamWaitEvent(s0, fan[FAN_L_DONE], 0));
    OG_HIP(hipStreamWaitEvent(s0, fan[FAN_PRODUCTS], 0));
    ProfScope ps_asm(ctx, PROF_ASSEMBLE, (double)s.sb);
    OG_TRY(assemble_g1_late(ctx, s.res(c, 3), s.res(c, 4), (size_t)s.sb, s.asm_tmp(c), proofs_sub, c.glv_d != nullptr));
    OG_STEP(ctx, "g16.assemble");
  } else {  // the side streams' G1 results; the G2 half is B's stream's (above)
    for (int e : {FAN_B1_DONE, FAN_A_DONE, FAN_L_DONE}) OG_HIP(hipStreamWaitEvent(s0, fan[e], 0));
    if (c.assembles()) {
      ProfScope ps_asm(ctx, PROF_ASSEMBLE, (double)s.sb);
      OG_TRY(assemble_g1(ctx, pk->consts1, rs_sub, s.res(c, 0), s.res(c, 1), s.res(c, 3), s.res(c, 4), (size_t)s.sb, s.asm_tmp(c), proofs_sub,
                         s.glv(c)));
      OG_STEP(ctx, "g16.assemble");
    }
  }
  if (asm_early) OG_HIP(hipStreamWaitEvent(s0, fan[FAN_A_DONE], 0));  // A's half of the proof
  OG_HIP(hipStreamWaitEvent(s0, ctx->ev1, 0));  // stream 0 ends after B's half too (scratch reuse by the next call)
  return OG_OK;
}

// ---- schedule 2: the stage pipeline --------------------------------------------------------------------------------------------
// A software pipeline over sub-batches on four streams, two scratch slots:
//   PREP stream (lanes[1])   witness generation, the three sparse products + the satisfiability check, the digit sorts of
//                            the A | B | L queries: memory- / latency-bound kernels with small register footprints
//   MATH stream (lanes[0])   quotient (NTT) and the five bucket accumulations, back to back: VALU-bound
//   AUX stream               the digit sort of h: it needs THIS sub-batch's quotient and is needed by its last accumulation, and
//                            here it does not queue behind the next sub-batch's preparation (which the prep stream was given first)
//   TAIL stream              each MSM's heavy buckets / reduction / combine (msm_run sends them to ctx->tail_stream), where
//                            they fill the ramp-down of the following accumulation; then the sub-batch's proof assembly
// prep(k + 1) runs under math(k).  All VALU-heavy kernels sit on ONE stream, in order.  (Round 2's first scheme alternated
// whole sub-batches between two symmetric lanes; once bucket accumulation moved to one-wave workgroups, a 300-register
// reduction kernel of one lane could wait for the whole length of the other lane's accumulation kernel -- up to 129 ms in
// the rocprof trace -- because every slot a finishing wave freed was refilled at once by a smaller-footprint wave.)
// Every query keeps its own sorted entries (sort slots 1, 3, 4; a shared wire list is sorted once: pk->sort_src) so that all
// three can be ready before the math stage needs them.  The slot (= scratch namespace and event set, ctx.h PipeEvent) is the
// pipeline's sub-batch counter mod 2, and the counter runs on across calls: the next call's first sub-batch must not take the
// slot this call's last one is still using, and it waits for what the slot's previous user recorded, whichever call that was.
// A slot is released in two steps: what the preparation overwrites (witnesses, A z / B z / C z, sorted digits) is last read by
// its previous user's heavy-bucket kernels (EV_PREP_FREE); the bucket sets and reduction levels that the late tail kernels work
// on are not touched before the math stage (EV_ASSEMBLED).  So TWO slots do what round 3's three did, same box, interleaved
// (profiles/r06b_ab_pipe_slots.txt); one slot less is ~35 GB of HBM at batch 1024.
// The quotient sits on the math stream, in front of the sub-batch's accumulations: beside the previous sub-batch's
// accumulations it loses (DESIGN.md 4.4 -- its ~37 ms per sub-batch on the math stream are the only windows in which the
// tails' big-register kernels find room).
static int issue_pipeline(const ProveCall& c, SubBatch& s) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  hipStream_t math = ctx->lanes[0], prep = ctx->lanes[1], aux = ctx->aux_lane, tail = ctx->tail_lane;
  s.slot = (int)(ctx->pipe_counter++ % og_ctx::PIPE_SLOTS);
  hipEvent_t* ev = ctx->pipe_ev[s.slot];
  auto on = [&](hipStream_t st) { ctx->stream = st; };
  auto rec = [&](int e) -> int { OG_HIP(hipEventRecord(ev[e], ctx->stream)); return OG_OK; };
  auto wait = [&](int e) -> int { OG_HIP(hipStreamWaitEvent(ctx->stream, ev[e], 0)); return OG_OK; };
  ctx->lane = s.slot;
  // ---------------- PREP ----------------
  on(prep);
  OG_TRY(wait(EV_PREP_FREE));
  OG_TRY(sub_front(c, s));
  OG_TRY(sub_rows(c, s));
  OG_TRY(rec(EV_ROWS));
  DigitSort ds_a, ds_b, ds_l, dh;
  OG_TRY(sub_sort(c, s, 1, 0, &ds_a));
  OG_TRY(rec(EV_SORT_A));
  if (pk->sort_src[1] == 0) ds_b = ds_a;  // same wire list (pk_load): the sorted entries serve both
  else OG_TRY(sub_sort(c, s, 3, 1, &ds_b));
  OG_TRY(rec(EV_SORT_B));
  if (pk->sort_src[2] == 0) ds_l = ds_a;
  else if (pk->sort_src[2] == 1) ds_l = ds_b;
  else OG_TRY(sub_sort(c, s, 4, 2, &ds_l));
  OG_TRY(rec(EV_SORT_L));
  // ---------------- QUOTIENT ----------------
  on(math);
  OG_TRY(wait(EV_ROWS));
  OG_TRY(sub_quotient(c, s));
  OG_TRY(rec(EV_QUOT));
  on(aux);
  OG_TRY(wait(EV_QUOT));
  OG_TRY(sub_sort_h(c, s, &dh));
  OG_TRY(rec(EV_SORT_H));
  // ---------------- MATH ----------------
  on(math);
  {
    struct TailGuard {
      og_ctx* c;
      ~TailGuard() { c->tail_stream = nullptr; c->msm_tag = 0; c->after_heavy_ev = nullptr; }
    } tail_guard{ctx};
    ctx->tail_stream = tail;
    OG_TRY(wait(EV_ASSEMBLED));  // the bucket sets / reduction levels of this slot: free once its previous user is assembled
    OG_TRY(wait(EV_SORT_A));
    ctx->msm_tag = 0;
    OG_TRY(msm_run(ctx, pk->a, ds_a, s.res(c, 0)));
    OG_TRY(wait(EV_SORT_B));
    ctx->msm_tag = 1;
    OG_TRY(msm_run(ctx, pk->b1, ds_b, s.res(c, 1)));
    ctx->msm_tag = 2;
    OG_TRY(msm_run(ctx, pk->b2, ds_b, s.res(c, 2)));
    OG_TRY(wait(EV_SORT_L));
    ctx->msm_tag = 3;
    OG_TRY(msm_l(c, s, ds_l));
    OG_TRY(wait(EV_SORT_H));
    // the H query is the sub-batch's last MSM: behind its heavy buckets nothing reads the slot's digit sorts (msm_run records it)
    ctx->after_heavy_ev = ev[EV_PREP_FREE];
    if (!pk->merge_lh) ctx->msm_tag = 4;  // (merged: the same tag, the same buckets)
    OG_TRY(msm_h(c, s, dh));
  }
  OG_STEP(ctx, "g16.msm");
  // Assembly needs every tail, and it is latency-bound (a few waves of scalar multiplications): it is queued on the tail
  // stream behind the last tail, so the math stream goes straight on to the next sub-batch's quotient instead of idling
  // through the H query's reduction and the assembly.  (Everything the math stream did for this sub-batch precedes one of
  // the tails, so "assembled" on the tail stream is also "math done".)
  on(tail);
  OG_TRY(sub_assemble(c, s));
  OG_TRY(rec(EV_ASSEMBLED));
  on(math);
  return OG_OK;
}

// ---- schedule 3: sub-batches one after the other on one stream ----------------------------------------------------------------
// og_set_lanes(1) (isolated kernel timings) runs every sub-batch on lanes[0].  With two lanes, sub-batches too small to fill
// the chip (a handful of requests each, below the pipeline's threshold) are latency-bound end to end: whole sub-batches then
// run side by side, sub-batch k on lanes[k & 1] in scratch namespace k & 1, which is worth ~1.5x (batch 8: 46 vs 68 ms).
// The witness queries share ONE set of sorted entries (sort slot 1: a third of the pipeline's scratch), interleaved with the MSMs.
static int issue_serial(const ProveCall& c, SubBatch& s, size_t sub_index) {
  og_ctx* ctx = c.ctx;
  const og_pk* pk = c.pk;
  s.slot = c.plan.sym ? (int)(sub_index & 1) : 0;
  ctx->lane = s.slot;
  ctx->stream = ctx->lanes[s.slot];
  OG_TRY(sub_front(c, s));
  OG_TRY(sub_rows(c, s));
  OG_TRY(sub_quotient(c, s));
  // A, then the queries that share A's wire list (their sort is A's: pk_load), then the rest; `held` = whose list the sorted
  // entries currently hold
  DigitSort ds, dh;
  int order[3] = {0, 1, 2}, held = -1;
  if (pk->sort_src[1] != 0 && pk->sort_src[2] == 0) std::swap(order[1], order[2]);
  for (int q : order) {
    if (pk->sort_src[q] != held) {
      OG_TRY(sub_sort(c, s, 1, q, &ds));
      held = pk->sort_src[q];
    }
    if (q == 0) OG_TRY(msm_run(ctx, pk->a, ds, s.res(c, 0)));
    if (q == 1) {
      OG_TRY(msm_run(ctx, pk->b1, ds, s.res(c, 1)));
      OG_TRY(msm_run(ctx, pk->b2, ds, s.res(c, 2)));
    }
    if (q == 2) OG_TRY(msm_l(c, s, ds));
  }
  OG_TRY(sub_sort_h(c, s, &dh));
  OG_TRY(msm_h(c, s, dh));
  OG_STEP(ctx, "g16.msm");
  return sub_assemble(c, s);
}

// everything is enqueued: the og_job, and one event per stream that marks the end of this call's work there
static int job_publish(const ProveCall& c, og_job** job_out) {
  og_ctx* ctx = c.ctx;
  og_job* job = new og_job();
  job->id = next_job_id();
  job->ctx = ctx; job->call_slot = c.call_slot; job->n = c.n; job->n_pub = c.pub_d ? c.pk->n_pub : 0;
  job->proofs = c.proofs; job->pub_out = c.pub_out; job->proofs_d = c.proofs_d; job->pub_d = c.pub_d; job->flags_d = c.flags;
  job->bad_kind = c.gen ? 2 : (c.trusted_z ? 0 : 1);
  if (c.gen) { job->gen_st = c.gen->st; job->gen_depth = c.gen->args.depth; }
  if (c.host_asm) {
    job->host_asm_pk = c.pk;
    for (int k = 0; k < 5; k++) job->res_d[k] = c.res[k];
    job->rs_h.assign(c.rs, c.rs + c.n * 64);
  }
  for (hipStream_t st : {ctx->lanes[0], ctx->lanes[1], ctx->tail_lane, ctx->aux_lane}) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess || hipEventRecord(e, st) != hipSuccess) {
      for (int k = 0; k < job->n_done; k++) (void)hipEventDestroy(job->done[k]);
      if (e) (void)hipEventDestroy(e);
      delete job;
      set_error("og_prove: could not record the completion events");
      return OG_ERR_HIP;  // (the caller's guard drains the streams)
    }
    job->done[job->n_done++] = e;
  }
  ctx->jobs[c.call_slot] = job;
  *job_out = job;
  return OG_OK;
}

static int prove_enqueue(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, const uint8_t* rs, uint8_t* proofs,
                         const StatementGen* gen, uint8_t* pub_out, og_job** job_out, const uint8_t* z_host = nullptr,
                         bool trusted_z = false, const WinShard* sh = nullptr) {
  *job_out = nullptr;
  ProveCall c{};
  c.ctx = ctx; c.pk = pk; c.n = n;
  c.gen = gen; c.z_host = z_host; c.z_d = z_d; c.trusted_z = trusted_z; c.sh = sh;
  c.rs = rs; c.proofs = proofs; c.pub_out = pub_out;
  // the first FREE call slot (not a toggle: a blocking call between a submit and its wait would flip a toggle back onto the
  // slot that is still occupied, and the next submit would be refused although only one call is in flight)
  c.call_slot = ctx->jobs[0] == nullptr ? 0 : 1;
  OG_REQUIRE(ctx->jobs[c.call_slot] == nullptr, "og_prove: two calls are already in flight on this context (og_job_wait or og_job_abandon one of them first)");
  OG_TRY(make_plan(ctx, pk, n, &c.plan));
  struct LaneGuard {  // an error return in the middle of the call leaves no work of it in flight (the next call reuses the
    og_ctx* c;        // scratch); on every path the ctx is back on lane 0
    bool ok = false;  // (everything is enqueued: the streams are left running)
    ~LaneGuard() {
      if (!ok) (void)drain_streams(c);
      c->lane = 0;
      c->stream = c->lanes[0];
      c->tail_stream = nullptr;
      c->sort_beside_acc = false;
    }
  } lane_guard{ctx};
  struct CallSize {  // the witness generator's host-chains bound looks at the call, not at the sub-batch it is handed
    og_ctx* c;
    ~CallSize() { c->call_requests = 0; }
  } call_size{ctx};
  ctx->call_requests = n;
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  OG_TRY(call_begin(c));
  const std::vector<int>& sizes = c.plan.plan;
  size_t g0 = 0;
  for (size_t k = 0; k < sizes.size(); g0 += sizes[k], k++) {
    SubBatch s{};
    s.g0 = g0;
    s.sb = sizes[k];
    if (c.plan.split) OG_TRY(issue_fan_out(c, s));
    else if (c.plan.pipe) OG_TRY(issue_pipeline(c, s));
    else OG_TRY(issue_serial(c, s, k));
  }
  OG_TRY(job_publish(c, job_out));
  lane_guard.ok = true;
  if (c.host_asm) assemble_fixed_on_host(pk, (*job_out)->rs_h.data(), n, (*job_out)->host_fixed);  // (the GPU is busy with the call's MSMs meanwhile)
  return OG_OK;
}

// OG_ERR_UNSATISFIED for witness g of the caller's batch: the ONE place the message is formed
static int unsatisfied(size_t g) {
  set_error("og_prove: witness " + std::to_string(g) + " does not satisfy the circuit (a row has a*b != c, or wire 0 is not 1)");
  return OG_ERR_UNSATISFIED;
}

// waits for the job's last kernels, copies proofs / flags / public inputs to the caller's buffers, frees the job
static int prove_finish(og_job* job, size_t* first_bad) {
  og_ctx* ctx = job->ctx;
  const size_t n = job->n;
  if (job->call_slot < 0) {  // completed inside the submit call
    auto& dj = ctx->done_jobs;
    dj.erase(std::remove(dj.begin(), dj.end(), job), dj.end());
    delete job;
    return OG_OK;
  }
  std::vector<uint32_t> fl(2 * n);
  struct Release {
    og_job* j;
    ~Release() {
      for (int k = 0; k < j->n_done; k++) (void)hipEventDestroy(j->done[k]);
      if (j->ctx->jobs[j->call_slot] == j) j->ctx->jobs[j->call_slot] = nullptr;
      delete j;
    }
  } release{job};
  for (int k = 0; k < job->n_done; k++) OG_HIP(hipStreamWaitEvent(ctx->copy_lane, job->done[k], 0));
  std::vector<uint8_t> res_h;
  if (job->host_asm_pk) {  // og_set_host_chains: the five query results come down, the host assembles (below)
    res_h.resize(n * 768);
    const size_t off[5] = {0, n * 128, n * 256, n * 512, n * 640}, len[5] = {128, 128, 256, 128, 128};
    for (int k = 0; k < 5; k++) OG_HIP(hipMemcpyAsync(res_h.data() + off[k], job->res_d[k], n * len[k], hipMemcpyDeviceToHost, ctx->copy_lane));
  } else if (job->proofs) OG_HIP(hipMemcpyAsync(job->proofs, job->proofs_d, n * 256, hipMemcpyDeviceToHost, ctx->copy_lane));  // (null: a sharded front)
  OG_HIP(hipMemcpyAsync(fl.data(), job->flags_d, n * 8, hipMemcpyDeviceToHost, ctx->copy_lane));
  if (job->pub_d) OG_HIP(hipMemcpyAsync(job->pub_out, job->pub_d, n * job->n_pub * 32, hipMemcpyDeviceToHost, ctx->copy_lane));
  OG_HIP(hipStreamSynchronize(ctx->copy_lane));
  if (job->host_asm_pk && job->proofs) assemble_on_host(job->host_asm_pk, job->rs_h.data(), job->host_fixed.data(), res_h.data(), n, job->proofs);
  // a malformed input (a non-canonical encoding) comes before "does not satisfy": OG_ERR_INVALID, naming the first offender
  if (job->bad_kind)
    for (size_t g = 0; g < n; g++) {
      const uint32_t b = fl[n + g];
      if (b == 0xffffffffu) continue;
      if (first_bad) *first_bad = g;
      if (job->bad_kind == 2)
        set_error(invalid_record_message(*job->gen_st, "og_" + std::string(job->gen_st->name) + "_prove", job->gen_depth, g, b));
      else
        set_error("og_prove: witness " + std::to_string(g) + ": wire " + std::to_string(b) + " is not a canonical Fr element (>= r)");
      return OG_ERR_INVALID;
    }
  for (size_t g = 0; g < n; g++)
    if (fl[g]) {
      if (first_bad) *first_bad = g;
      return unsatisfied(g);
    }
  return OG_OK;
}

// blocking form: enqueue + finish
static int prove_batch_impl(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, const uint8_t* rs, uint8_t* proofs,
                            size_t* first_bad, const StatementGen* gen, uint8_t* pub_out, bool trusted_z = false) {
  if (n == 0) return OG_OK;
  og_job* job = nullptr;
  OG_TRY(prove_enqueue(ctx, pk, z_d, n, rs, proofs, gen, pub_out, &job, nullptr, trusted_z));
  return prove_finish(job, first_bad);
}

int prove_batch_device(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, const uint8_t* rs, uint8_t* proofs,
                       size_t* first_bad) {
  return prove_batch_impl(ctx, pk, z_d, n, rs, proofs, first_bad, nullptr, nullptr);
}

// host witnesses: staged through a device buffer one sub-batch-sized slab at a time
int prove_batch_host(og_ctx* ctx, const og_pk* pk, const uint8_t* z, size_t n, const uint8_t* rs, uint8_t* proofs) {
  if (n == 0) return OG_OK;
  // ONE call: every sub-batch's witnesses are copied into its scratch slot by the prep stream (prove_enqueue, z_host), so
  // the PCIe traffic of sub-batch k + 1 (8.4 MB per 2^18-wire witness) runs under the accumulations of sub-batch k.
  // (Rounds 1-2 copied a 4 GiB slab, then proved it, then copied the next: -7 % against resident witnesses,
  // profiles/r03_host_boundary.json.)
  og_job* job = nullptr;
  OG_TRY(prove_enqueue(ctx, pk, nullptr, n, rs, proofs, nullptr, nullptr, &job, z));
  return prove_finish(job, nullptr);
}

// inputs (withdraw circuit records) -> proofs: witness generation fused into the lanes (withdraw_prove_batch, below)
// witnesses are generated inside the pipeline from this many wire values per sub-batch on (OG_GEN_MIN: test hook)
static size_t gen_threshold() { return (size_t)OG_HOOK_INT("OG_GEN_MIN", (long long)1 << 26); }
// Witnesses inside prove_enqueue (on stream 0, the queries' streams waiting for an event) instead of a slab up front with the host
// waiting for it: for big statements (a sub-batch proves for hundreds of ms) -- and for every call that fits ONE sub-batch, whose
// schedule is the fan-out: there the host's wait was the walk's whole length (3.4 ms of one request), and the ~80 launches of the
// queries were issued only after it -- 0.2-0.4 ms of launch latency in front of every stream.  Inside, they are queued while the
// walk runs.  (OG_GEN_ONE_SUB=0: the slab form, hooks builds.)
static bool gen_inside(const og_ctx* ctx, const og_pk* pk, size_t n, size_t sb) {
  (void)ctx;
  return sb * pk->m >= gen_threshold() || (n <= sb && OG_HOOK_INT("OG_GEN_ONE_SUB", 1) != 0);
}

int job_wait(og_job* job) { return prove_finish(job, nullptr); }

// the events that mark the end of the job's work on each stream (none for a job that completed inside its submit call)
int job_done_events(og_job* job, hipEvent_t* out) {
  if (job->call_slot < 0) return 0;
  for (int k = 0; k < job->n_done; k++) out[k] = job->done[k];
  return job->n_done;
}

// is `job` a handle this context handed out and has not yet consumed?  (pointer comparison only: never dereferences it)
bool job_is_live(og_ctx* ctx, og_job* job) {
  if (job == nullptr) return false;
  if (ctx->jobs[0] == job || ctx->jobs[1] == job) return true;
  return std::find(ctx->done_jobs.begin(), ctx->done_jobs.end(), job) != ctx->done_jobs.end();
}

// one waiter per job (capi.hip og_job_wait): set / clear the flag; returns the PREVIOUS state; *id_out = the job's serial number
bool job_mark_waiting(og_job* job, bool on, uint64_t* id_out) {
  const bool was = job->waiting;
  if (!(on && was)) job->waiting = on;
  if (id_out) *id_out = job->id;
  return was;
}
bool job_same(og_job* job, uint64_t id) { return job->id == id; }
bool job_is_waited_for(og_job* job) { return job->waiting; }
bool ctx_has_waiters(og_ctx* ctx) {
  for (og_job* j : {ctx->jobs[0], ctx->jobs[1]})
    if (j && j->waiting) return true;
  for (og_job* j : ctx->done_jobs)
    if (j && j->waiting) return true;
  return false;
}

// og_job_abandon: the caller no longer wants the results (its buffers may be gone).  Waits until the job's last kernels are
// done -- they write device scratch the next call reuses -- copies nothing out, frees the call slot and the handle.
int job_abandon(og_job* job) {
  og_ctx* ctx = job->ctx;
  if (job->call_slot < 0) {
    auto& dj = ctx->done_jobs;
    dj.erase(std::remove(dj.begin(), dj.end(), job), dj.end());
    delete job;
    return OG_OK;
  }
  hipError_t first = hipSuccess;
  for (int k = 0; k < job->n_done; k++) {
    const hipError_t e = hipEventSynchronize(job->done[k]);
    if (e != hipSuccess && first == hipSuccess) first = e;
    (void)hipEventDestroy(job->done[k]);
  }
  if (ctx->jobs[job->call_slot] == job) ctx->jobs[job->call_slot] = nullptr;
  delete job;
  OG_HIP(first);
  return OG_OK;
}

// ---- records -> proofs, every statement (statements.h) -------------------------------------------------------------------------
// the key must have the wires and the public inputs of the statement at these arguments: "og_<st>_<entry>: the key is not for ..."
static int statement_key_ok(const Statement& st, const StatementArgs& a, const og_pk* pk, const char* entry) {
  uint64_t shp[3];
  OG_TRY(records_shape_query(st, a, shp));
  OG_REQUIRE(shp[0] == pk->m && shp[2] == pk->n_pub, "og_" + std::string(st.name) + "_" + entry + ": the key is not for " + st.key_noun);
  return OG_OK;
}

// A slab: the witnesses generated in ONE launch up front and proved from one buffer -- 16 GiB of wires, at most 65 535 (a record's
// index is grid.y of its check).  OG_SLAB_MAX (hooks builds) lowers the bound: tests/statement_slab_cases.py reaches a second slab with
// it.  A window-sharded call is one slab, so there the hook lowers the call's cap too ("at most N proofs ... per window-sharded call").
static size_t slab_limit(const og_pk* pk) {
  const size_t by_bytes = std::max<size_t>(1, ((size_t)16 << 30) / (pk->m * 32));
  return std::min(std::min<size_t>(65535, by_bytes), (size_t)std::max<long long>(1, OG_HOOK_INT("OG_SLAB_MAX", 65535)));
}

// one slab's witnesses in z_d: the records checked (blocking; `base` = index of record 0 in the caller's batch), the walk launched,
// the stream idle -- every stream of the prover reads the slab
static int slab_witnesses(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* records_d, size_t cnt, size_t base,
                          uint8_t* z_d) {
  OG_TRY(records_ok(st, ctx, a, records_d, cnt, base));
  OG_TRY(st.witness(st, ctx, a, records_d, cnt, z_d));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

// The witness generators are latency-bound (one lane, or one wave, walks a request's hashes whatever the launch size), and a sub-batch
// of a small circuit proves in about the same time: so whole slabs of witnesses in one launch, then the ordinary batched prover.  For
// join, the prover's row check is what answers OG_ERR_UNSATISFIED for two notes under different roots: the witness carries note a's
// root in wire 1.
static int prove_slabs(const Statement& st, og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n,
                       const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out) {
  if (n == 0) return OG_OK;
  const size_t rec = record_bytes(st, a.depth), slab = std::min(n, slab_limit(pk));
  uint8_t* z_d = nullptr;
  OG_TRY(arena_get(ctx, "g16.zall", slab * pk->m * 32, (void**)&z_d));
  for (size_t g0 = 0; g0 < n; g0 += slab) {
    const size_t cnt = std::min(slab, n - g0);
    OG_TRY(slab_witnesses(st, ctx, a, inputs_d + g0 * rec, cnt, g0, z_d));
    size_t bad = 0;
    const int r = prove_batch_impl(ctx, pk, z_d, cnt, rs + g0 * 64, proofs + g0 * 256, &bad, nullptr,
                                   pub_out ? pub_out + g0 * pk->n_pub * 32 : nullptr, true);  // (our own generator's wires are canonical)
    if (r == OG_ERR_UNSATISFIED) return unsatisfied(g0 + bad);
    if (r != OG_OK) return r;
  }
  return OG_OK;
}

int statement_prove_batch(const Statement& st, og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n,
                          const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out) {
  OG_TRY(statement_key_ok(st, a, pk, "prove_batch_d"));
  return prove_slabs(st, ctx, pk, a, inputs_d, n, rs, proofs, pub_out);
}

// Withdraw: big circuits hide the walk inside the lanes (a sub-batch proves for hundreds of ms), and so does every call of one
// sub-batch (gen_inside); the rest goes slab by slab like every other statement.
int withdraw_prove_batch(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                         uint8_t* proofs, uint8_t* pub_out) {
  OG_TRY(statement_key_ok(ST_WITHDRAW, a, pk, "prove_batch_d"));
  if (gen_inside(ctx, pk, n, (size_t)choose_sub_batch(ctx, pk, n))) {
    const StatementGen gen{&ST_WITHDRAW, a, inputs_d};
    return prove_batch_impl(ctx, pk, nullptr, n, rs, proofs, nullptr, &gen, pub_out);
  }
  return prove_slabs(ST_WITHDRAW, ctx, pk, a, inputs_d, n, rs, proofs, pub_out);
}

// Enqueue-only form of withdraw_prove_batch: returns a job whose results og_job_wait delivers.  Circuits whose witnesses are
// generated inside the pipeline (the large ones) are really left running; for small circuits (whole-slab witness
// generation up front, shared staging) the call completes here and the job only carries the status.
int withdraw_prove_batch_submit(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                                uint8_t* proofs, uint8_t* pub_out, og_job** job_out) {
  *job_out = nullptr;
  OG_TRY(statement_key_ok(ST_WITHDRAW, a, pk, "prove_batch_submit_d"));
  OG_REQUIRE(n >= 1, "og_withdraw_prove_batch_submit_d: empty batch");
  if (gen_inside(ctx, pk, n, (size_t)choose_sub_batch(ctx, pk, n))) {
    const StatementGen gen{&ST_WITHDRAW, a, inputs_d};
    return prove_enqueue(ctx, pk, nullptr, n, rs, proofs, &gen, pub_out, job_out);
  }
  OG_TRY(withdraw_prove_batch(ctx, pk, a, inputs_d, n, rs, proofs, pub_out));
  og_job* job = new og_job();  // nothing left to wait for
  job->id = next_job_id();
  job->ctx = ctx;
  job->call_slot = -1;
  ctx->done_jobs.push_back(job);
  *job_out = job;
  return OG_OK;
}

// ---- window-sharded proving: the two halves (WinShard above) -------------------------------------------------------------------
// Front half, enqueue only: this rank's partial sums of the five queries of n proofs into partials_d (n x PARTIAL_BYTES, device,
// the caller's), everything left running on the context's streams; the job carries the boundary flags and the public inputs
// (og_job_wait semantics: prove_finish reports a malformed record / an unsatisfied witness exactly as the unsharded call does).
int withdraw_prove_partials_enqueue(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, int win_rank,
                                    int win_world, uint8_t* partials_d, uint8_t* pub_out, og_job** job_out) {
  *job_out = nullptr;
  OG_TRY(statement_key_ok(ST_WITHDRAW, a, pk, "prove_partials"));
  OG_REQUIRE(n >= 1, "og_withdraw_prove_partials: empty batch");
  OG_REQUIRE(win_world >= 1 && win_world <= pk->a->nwin && win_rank >= 0 && win_rank < win_world,
             "og_withdraw_prove_partials: bad window shard (rank, world): at most one rank per window");
  const WinShard sh{win_rank, win_world, partials_d};
  if (gen_inside(ctx, pk, n, (size_t)choose_sub_batch(ctx, pk, n))) {
    const StatementGen gen{&ST_WITHDRAW, a, inputs_d};
    return prove_enqueue(ctx, pk, nullptr, n, nullptr, nullptr, &gen, pub_out, job_out, nullptr, false, &sh);
  }
  // small statements: the whole call's witnesses in one launch up front (prove_slabs); a sharded call is one slab
  const size_t slab = slab_limit(pk);
  OG_REQUIRE(n <= slab, "og_withdraw_prove_partials: at most " + std::to_string(slab) + " proofs of this statement per window-sharded call");
  uint8_t* z_d = nullptr;
  OG_TRY(arena_get(ctx, "g16.zall", n * pk->m * 32, (void**)&z_d));
  OG_TRY(slab_witnesses(ST_WITHDRAW, ctx, a, inputs_d, n, 0, z_d));
  return prove_enqueue(ctx, pk, z_d, n, nullptr, nullptr, nullptr, pub_out, job_out, nullptr, true, &sh);
}

// the same for caller-supplied witnesses (device, n x m x 32 B canonical)
int prove_partials_enqueue(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, int win_rank, int win_world, uint8_t* partials_d,
                           og_job** job_out) {
  *job_out = nullptr;
  OG_REQUIRE(n >= 1, "og_prove_partials: empty batch");
  OG_REQUIRE(win_world >= 1 && win_world <= pk->a->nwin && win_rank >= 0 && win_rank < win_world,
             "og_prove_partials: bad window shard (rank, world): at most one rank per window");
  const WinShard sh{win_rank, win_world, partials_d};
  return prove_enqueue(ctx, pk, z_d, n, nullptr, nullptr, nullptr, nullptr, job_out, nullptr, false, &sh);
}

// every stream of the job's call -> `st` waits for it (the in-library all-gather is issued behind the front half, stream-ordered)
int job_join_stream(og_job* job, hipStream_t st) {
  if (job->call_slot < 0) return OG_OK;
  for (int k = 0; k < job->n_done; k++) OG_HIP(hipStreamWaitEvent(st, job->done[k], 0));
  return OG_OK;
}

// Back half: gathered_d = `world` blocks of n x PARTIAL_BYTES (rank-major, every rank's partials_d as the all-gather left them).
// Adds the ranks' shares query by query, assembles the n proofs with the blinding (r, s) and copies them out.  Enqueued on
// lanes[0] behind whatever the caller ordered there (the all-gather); blocking.
int prove_from_partials(og_ctx* ctx, const og_pk* pk, const uint8_t* gathered_d, int world, size_t n, const uint8_t* rs, uint8_t* proofs) {
  OG_REQUIRE(world >= 1 && n >= 1 && n <= 65535, "og_prove_from_partials: bad world / batch");
  ctx->lane = 0;
  ctx->stream = ctx->lanes[0];
  uint8_t *res[5], *rs_d, *proofs_d, *asm_tmp, *glv_d = nullptr;
  const size_t rank_stride = n * PARTIAL_BYTES;
  const size_t off[5] = {0, n * 128, 4 * n * 128, 2 * n * 128, 3 * n * 128};  // A | B1 | (B2 last) | L | H: the order of `res`
  if (world == 1) {
    for (int k = 0; k < 5; k++) res[k] = const_cast<uint8_t*>(gathered_d) + off[k];
  } else {
    ProfScope ps(ctx, PROF_REDUCE_G1, 0.0);
    for (int k = 0; k < 5; k++) {
      OG_TRY(arena_get(ctx, ("g16.sh.res" + std::to_string(k)).c_str(), n * (k == 2 ? 256 : 128), (void**)&res[k]));
      OG_TRY(msm_sum_ranks(ctx, k == 2, gathered_d + off[k], rank_stride, world, (int)n, res[k]));
    }
  }
  std::vector<uint8_t> glv_h;
  glv_halves(rs, n, glv_h);
  const size_t asm_lanes = glv_h.empty() ? 4 : 8;
  OG_TRY(arena_get(ctx, "g16.sh.rs", n * 64, (void**)&rs_d));
  OG_TRY(arena_get(ctx, "g16.sh.proofs", n * 256, (void**)&proofs_d));
  OG_TRY(arena_get(ctx, "g16.sh.asm", n * asm_lanes * 128 * 17, (void**)&asm_tmp));
  if (!glv_h.empty()) OG_TRY(arena_get(ctx, "g16.sh.glv", n * 128, (void**)&glv_d));
  OG_HIP(hipMemcpyAsync(rs_d, rs, n * 64, hipMemcpyHostToDevice, ctx->stream));
  if (glv_d) OG_HIP(hipMemcpyAsync(glv_d, glv_h.data(), n * 128, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps_asm(ctx, PROF_ASSEMBLE, (double)n);
    OG_TRY(assemble_g1(ctx, pk->consts1, rs_d, res[0], res[1], res[3], res[4], n, asm_tmp, proofs_d, glv_d));
    OG_TRY(assemble_g2(ctx, pk->consts2, pk->fb_delta2, rs_d, res[2], n, proofs_d, n <= 1024));  // (a waited-for tail: a wave per proof)
  }
  OG_HIP(hipMemcpyAsync(proofs, proofs_d, n * 256, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));  // (glv_h, pageable rs: the host buffers of the async copies outlive them)
  return OG_OK;
}

}  // namespace og
