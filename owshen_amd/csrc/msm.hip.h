// Internal interface of the Pippenger MSM (msm.hip), shared with the Groth16 prover (groth16.hip).
#pragma once
#include "ctx.h"

struct og_bases {
  int is_g2 = 0;
  size_t n = 0;        // points per window table
  int c = 16;          // window bits (signed digits -> 2^(c-1) buckets)
  int nwin = 16;       // ceil(255 / c)
  int precomp = 0;     // 1: tab holds nwin tables, tab[k][i] = 2^(c k) P_i  (single bucket set)
  uint8_t* tab_d = nullptr;  // affine, Montgomery form; (precomp ? nwin : 1) * n points
  int device = 0;
};

namespace og {

// Sorted signed-digit decomposition of `batch` scalar vectors (shared by every MSM over the
// same scalars, e.g. Groth16's A / B1 / B2 / L queries all consume the witness z).
struct DigitSort {
  size_t n = 0;
  int batch = 0;
  int c = 16, nwin = 16, precomp = 0;
  uint32_t own_mask = 0xffffffffu;  // bit k: window k is accumulated by this rank (window-sharded MSM; all ones = every window)
  int n_own = 16;          // popcount(own_mask & windows)
  size_t nkeys = 0;        // bucket slots per batch item = (precomp ? 1 : n_own) * 2^(c-1)
  size_t ecap = 0;         // entry capacity per batch item = n * nwin
  uint32_t* offsets = nullptr;  // [batch][nkeys + 1] exclusive prefix of bucket sizes
  uint32_t* cursor = nullptr;   // [batch][nkeys] scatter cursors
  uint32_t* entries = nullptr;  // [batch][ecap]: (table_index << 1) | negate
  uint32_t* order = nullptr;    // [batch][nkeys]: bucket ids by descending size (lane -> bucket map of the
                                // accumulation kernel, so the 64 lanes of a wave carry equal work)
};

size_t msm_pick_c(size_t n);
size_t msm_pick_query_c(size_t n);
int msm_nwin(int c);

// workspace-managed (ctx arena); valid until the next digit_sort on the same slot
// map_d (optional, device, n x u32): entry i takes the scalar at index map_d[i] of each vector -- density
// compaction: a query whose bases are mostly the point at infinity is stored compacted and visits only the
// wires it has a base for (what bellman calls the query density).
int msm_digit_sort(og_ctx* ctx, int slot, const uint8_t* scalars_d, size_t scalar_stride_bytes, size_t n,
                   const uint32_t* map_d, int batch, int c, int precomp, DigitSort* out);

// same, restricted to the windows k with k % win_world == win_rank (window-sharded MSM over several GPUs)
int msm_digit_sort_windows(og_ctx* ctx, int slot, const uint8_t* scalars_d, size_t scalar_stride_bytes, size_t n,
                           const uint32_t* map_d, int batch, int c, int precomp, int win_rank, int win_world, DigitSort* out);

// bucket accumulation + reduction; result[g] (XYZZ, Montgomery) for g < batch written to out_d
// (G1: 128 B each, G2: 256 B each).
int msm_run(og_ctx* ctx, const og_bases* bases, const DigitSort& ds, uint8_t* out_xyzz_d);
// Two queries whose results are only ever ADDED (Groth16's C = sum z_i L_i + sum h_j H_j) are ONE MSM over the concatenated
// points: they share a bucket set -- same window bits, same batch, G1 -- and with it one bucket reduction, one heavy-bucket tail
// and one window combine per proof instead of two.  The two halves keep their own tables and digit sorts (the scalars come
// from different buffers at different times):
//   MSM_FIRST   accumulate into a fresh bucket set named by ctx->msm_tag, fold the heavy buckets in, stop (out is not written)
//   MSM_SECOND  same ctx->lane / msm_tag: add to those buckets, then heavy buckets (added in), reduction, combine -> out
enum MsmPhase { MSM_FULL = 0, MSM_FIRST = 1, MSM_SECOND = 2 };
int msm_run_phase(og_ctx* ctx, const og_bases* bases, const DigitSort& ds, uint8_t* out_xyzz_d, int phase);
// Window-sharded form: this rank's partial result as an array of msm_partial_slots(bases) XYZZ points per batch item --
// one point per window (the points of windows this rank does not own are the point at infinity) for plain bases, ONE
// partial sum for precomputed tables.  After an all-gather of every rank's array, msm_combine adds the ranks' arrays
// slot by slot and runs Horner over the windows: out[g] = sum_k 2^(c k) sum_r partial[r][g][k].
int msm_partial_slots(const og_bases* bases);
int msm_run_partial(og_ctx* ctx, const og_bases* bases, const DigitSort& ds, uint8_t* partial_xyzz_d);
int msm_combine(og_ctx* ctx, const og_bases* bases, const uint8_t* gathered_xyzz_d, int world, int batch, uint8_t* out_xyzz_d);

// out[g] = sum_r gathered[r * rank_stride + g * sizeof(XYZZ)] for g < batch: the ranks' partial sums of one query, added
int msm_sum_ranks(og_ctx* ctx, int is_g2, const uint8_t* gathered_xyzz_d, size_t rank_stride, int world, int batch, uint8_t* out_xyzz_d);

int bases_create(og_ctx* ctx, int is_g2, const uint8_t* points_d, size_t n, int c, int precomp, og_bases** out);
void bases_destroy(og_bases* b);

// out (canonical affine bytes, device) = to_affine(xyzz[i]) for i < count
int xyzz_to_affine_bytes(og_ctx* ctx, int is_g2, const uint8_t* xyzz_d, uint8_t* out_d, size_t count);

// arena: named scratch buffers that grow on demand and live until og_shutdown
int arena_get(og_ctx* ctx, const char* name, size_t bytes, void** out);
bool arena_has(og_ctx* ctx, const char* name);

// ---- the per-group instantiations (msm_g1.hip, msm_g2.hip) --------------------------------------------------------------------------
// what msm.hip dispatches to on og_bases::is_g2 ...
int msm_run_g1(og_ctx* ctx, const og_bases* b, const DigitSort& ds, uint8_t* out, bool partial, int phase);
int msm_run_g2(og_ctx* ctx, const og_bases* b, const DigitSort& ds, uint8_t* out, bool partial, int phase);
int msm_combine_g1(og_ctx* ctx, const og_bases* b, const uint8_t* gathered, int world, int batch, uint8_t* out);
int msm_combine_g2(og_ctx* ctx, const og_bases* b, const uint8_t* gathered, int world, int batch, uint8_t* out);
int msm_sum_ranks_g1(og_ctx* ctx, const uint8_t* gathered, size_t rank_stride, int world, int batch, uint8_t* out);
int msm_sum_ranks_g2(og_ctx* ctx, const uint8_t* gathered, size_t rank_stride, int world, int batch, uint8_t* out);
int bases_fill_g1(og_ctx* ctx, og_bases* b, const uint8_t* pts);
int bases_fill_g2(og_ctx* ctx, og_bases* b, const uint8_t* pts);
int xyzz_to_affine_bytes_g1(og_ctx* ctx, const uint8_t* in, uint8_t* out, size_t n);
int xyzz_to_affine_bytes_g2(og_ctx* ctx, const uint8_t* in, uint8_t* out, size_t n);

// ... and what the prover (groth16.hip) calls: fixed-base multiplication, point import, proof assembly (ecmul_impl.hip.h)
// tab_d: 64 x 16 x 128 B fixed-base table of the point at base_mont_d (see k_fixed_table)
int fixed_table_g1(og_ctx* ctx, const uint8_t* base_mont_d, uint8_t* tab_d);
int fixed_table_g2(og_ctx* ctx, const uint8_t* base_mont_d, uint8_t* tab_d);
int scalar_mul_fixed_g1(og_ctx* ctx, const uint8_t* tab_d, const uint8_t* k_d, size_t n, uint8_t* out_d);
int scalar_mul_fixed_g2(og_ctx* ctx, const uint8_t* tab_d, const uint8_t* k_d, size_t n, uint8_t* out_d);
int import_points_g1(og_ctx* ctx, const uint8_t* in_d, uint8_t* out_d, size_t n);
int import_points_g2(og_ctx* ctx, const uint8_t* in_d, uint8_t* out_d, size_t n);
// proofs_d[g][0:64] = A, [192:256] = C   (tmp_d: n x 4 x 17 x 128 B scratch: four products + their four window tables per proof)
// glv_d (optional): n x 4 x 32 B, the GLV halves of r, r s, s, r per proof (glv.h) -- then eight lanes per proof walk
// half-length chains (tmp_d: n x 8 x 17 x 128 B)
int assemble_g1(og_ctx* ctx, const uint8_t* consts_d, const uint8_t* rs_d, const uint8_t* res_a, const uint8_t* res_b1,
                const uint8_t* res_l, const uint8_t* res_h, size_t n, uint8_t* tmp_d, uint8_t* proofs_d, const uint8_t* glv_d);
// assemble_g1 in two parts (ecmul_impl.hip.h), each on the ctx's current stream: the products (need the A and B1 results), then A's
// sum (`early`); C's sum (`late`: needs the L and H results and the PRODUCTS -- `products_done`, if given, is recorded between the two)
int assemble_g1_early(og_ctx* ctx, const uint8_t* consts_d, const uint8_t* rs_d, const uint8_t* res_a, const uint8_t* res_b1, size_t n,
                      uint8_t* tmp_d, uint8_t* proofs_d, const uint8_t* glv_d, hipEvent_t products_done);
int assemble_g1_late(og_ctx* ctx, const uint8_t* res_l, const uint8_t* res_h, size_t n, const uint8_t* tmp_d, uint8_t* proofs_d, bool glv);
// proofs_d[g][64:192] = B
int assemble_g2(og_ctx* ctx, const uint8_t* consts_d, const uint8_t* fb_tab_d, const uint8_t* rs_d, const uint8_t* res_b2, size_t n,
                uint8_t* proofs_d, bool wave_per_proof = false);

}  // namespace og
