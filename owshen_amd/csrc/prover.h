// What the Groth16 prover (groth16.hip) and the transforms under it (ntt.hip) offer to the other units: the entry points (capi.hip),
// the N-device layer (multi.hip), key generation (keygen.hip).  og_pk is defined in groth16.hip and opaque everywhere else.
#pragma once
#include "ctx.h"

namespace og {

// ---- ntt.hip ------------------------------------------------------------------------------------------------------------------------
// consts buffer of the size-2^log_n domain (see NttPlan): used by the Groth16 setup helpers
int ntt_domain_consts(og_ctx* ctx, int log_n, uint8_t** consts_d);
// Standalone transform on canonical data (C ABI og_ntt_fr_d): out-of-place into out_d.
int ntt_canonical(og_ctx* ctx, const uint8_t* in_d, uint8_t* out_d, int log_n, int batch, int inverse, int coset);
// H-polynomial on device buffers: a, b, c Montgomery evaluations (destroyed), tmp scratch,
// h_out canonical coefficients; all batch x d x 32 B
int h_poly_device(og_ctx* ctx, uint8_t* a, uint8_t* b, uint8_t* c, uint8_t* tmp, uint8_t* h_out, int log_d, int batch, int coset_form);
// C ABI og_h_poly_d: canonical evaluations in (not modified), canonical coefficients out
int h_poly_canonical(og_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* c, int log_d, int batch, uint8_t* h_out);

// ---- groth16.hip: the helpers of key generation ---------------------------------------------------------------------------------------
int spmv_canonical(og_ctx* ctx, const uint32_t* ptr_d, const uint32_t* col_d, const uint8_t* val_d, size_t n_rows,
                   const uint8_t* x_d, uint8_t* out_d);
int lagrange_evals(og_ctx* ctx, int log_d, const uint8_t tau[32], uint8_t* out_d);
int scalar_mul_fixed(og_ctx* ctx, int is_g2, const uint8_t* base_host, const uint8_t* scalars_d, size_t n, uint8_t* out_d);

// ---- ptau.hip -------------------------------------------------------------------------------------------------------------------------
// n canonical affine points on the host, checked on the device: *flags |= 1 a coordinate >= q, |= 2 a point off its curve
int points_on_curve(og_ctx* ctx, int is_g2, const uint8_t* points, size_t n, uint32_t* flags);

// ---- groth16.hip: the proving key (the serialized key: key_blob.h) ----------------------------------------------------------------------
// rows (optional, rows_len bytes): the key's OWPR0001 row-basis extension; a wrong one is refused, OG_ERR_INVALID
int pk_load(og_ctx* ctx, const uint8_t* blob, size_t len, const uint8_t* rows, size_t rows_len, og_pk** out);
void pk_destroy(og_pk* pk);
// the rule of pk_load: does a query with rows_q non-empty rows and wires_q bases run over the rows?  (key generation asks too:
// it makes no extension that no load would use)
bool row_form_pays(size_t rows_q, size_t wires_q);
// what each of the five queries A | B1 | B2 | L | H runs: form (0 wires, 1 rows), points, window bits, table number -- 4 words each
void pk_query_form(const og_pk* pk, uint64_t out[20]);
// out[0..3] = n_wires, n_pub, log_d, n_rows: the key's header
void pk_info(const og_pk* pk, uint64_t out[4]);
// out[0..3] = window bits of the A, B (G1 and G2 copies), L and H queries' precomputed tables (msm_pick_query_c)
void pk_windows(const og_pk* pk, uint64_t out[4]);
// out[0..2] = bases kept by the A, B (G1 and G2 copies) and L queries after density compaction; out[3] = the H query's d - 1
void pk_density(const og_pk* pk, uint64_t out[4]);
// HBM bytes of the resident key: CSR matrices, the five queries' per-window tables, wire maps, constants
uint64_t pk_bytes(const og_pk* pk);

// ---- groth16.hip: proving ---------------------------------------------------------------------------------------------------------------
// is glv.h's (lambda, beta) a pair?  Checked once per process; on failure the GLV path is off
bool glv_pair_ok();
// sizes_out[0 .. *count_out) = the sub-batches a call of n proofs is cut into; *mode_out = 0 one stream, serial; 1 a call of <= 16 requests, its queries
// fanned out over the streams; 2 whole sub-batches side by side on two streams; 3 the stage pipeline
int prove_plan(og_ctx* ctx, const og_pk* pk, size_t n, uint32_t* sizes_out, size_t cap, size_t* count_out, int* mode_out);
// blocking form: enqueue + finish
int prove_batch_device(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, const uint8_t* rs, uint8_t* proofs,
                       size_t* first_bad);
// host witnesses: staged through a device buffer one sub-batch-sized slab at a time
int prove_batch_host(og_ctx* ctx, const og_pk* pk, const uint8_t* z, size_t n, const uint8_t* rs, uint8_t* proofs);
// the front half of a window-sharded call for caller-supplied witnesses (device, n x m x 32 B canonical)
int prove_partials_enqueue(og_ctx* ctx, const og_pk* pk, const uint8_t* z_d, size_t n, int win_rank, int win_world, uint8_t* partials_d,
                           og_job** job_out);
// Back half: gathered_d = `world` blocks of n x PARTIAL_BYTES (rank-major, every rank's partials_d as the all-gather left them).
// Adds the ranks' shares query by query, assembles the n proofs with the blinding (r, s) and copies them out.  Enqueued on
// lanes[0] behind whatever the caller ordered there (the all-gather); blocking.
int prove_from_partials(og_ctx* ctx, const og_pk* pk, const uint8_t* gathered_d, int world, size_t n, const uint8_t* rs, uint8_t* proofs);

// ---- groth16.hip: jobs (one enqueued prove_batch call: ctx.h) ---------------------------------------------------------------------------
int job_wait(og_job* job);
// the events that mark the end of the job's work on each stream (none for a job that completed inside its submit call)
int job_done_events(og_job* job, hipEvent_t* out);
// is `job` a handle this context handed out and has not yet consumed?  (pointer comparison only: never dereferences it)
bool job_is_live(og_ctx* ctx, og_job* job);
// one waiter per job (capi.hip og_job_wait): set / clear the flag; returns the PREVIOUS state; *id_out = the job's serial number
bool job_mark_waiting(og_job* job, bool on, uint64_t* id_out);
bool job_same(og_job* job, uint64_t id);
bool job_is_waited_for(og_job* job);
bool ctx_has_waiters(og_ctx* ctx);
// og_job_abandon: the caller no longer wants the results (its buffers may be gone).  Waits until the job's last kernels are
// done -- they write device scratch the next call reuses -- copies nothing out, frees the call slot and the handle.
int job_abandon(og_job* job);
// every stream of the job's call -> `st` waits for it (the in-library all-gather is issued behind the front half, stream-ordered)
int job_join_stream(og_job* job, hipStream_t st);

}  // namespace og
