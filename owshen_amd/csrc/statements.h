// The statements between their translation units: what witness.hip (kernels, boundary checks, witness launches), keygen.hip (the R1CS
// builders), groth16.hip (records -> proofs) and capi.hip (the entry points) call of one another, declared once.
//
// withdraw and deposit are plain functions.  split, join and transfer -- the "record statements": a record of n_rec fields and
// `paths` blocks of `depth` siblings, a shape that depends on the depth alone, a lane-local walk for batches and a wave-wide one for
// small calls -- are one descriptor each, and everything that does not depend on the statement is written once over it
// ("adding a record statement").
#pragma once
#include "ctx.h"
#include "msm.hip.h"  // arena_get

namespace og {

// ---- withdraw ---------------------------------------------------------------------------------------------------------------------
int withdraw_shape_query(int depth, uint64_t n_pad3, uint64_t n_pad2, uint64_t out[3]);                                              // witness.hip
int withdraw_check_records(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint32_t* bad_d);
const char* withdraw_field_name(uint32_t f);
int withdraw_witness(og_ctx* ctx, int depth, uint64_t n_pad3, uint64_t n_pad2, const uint8_t* inputs_d, size_t n, uint8_t* out_d);
int withdraw_records_ok(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, size_t base);                                     // groth16.hip
int withdraw_prove_batch(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2, const uint8_t* inputs_d, size_t n,
                         const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out);
int withdraw_prove_batch_submit(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2, const uint8_t* inputs_d, size_t n,
                                const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out, og_job** job_out);
int withdraw_prove_partials_enqueue(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2, const uint8_t* inputs_d, size_t n,
                                    int win_rank, int win_world, uint8_t* partials_d, uint8_t* pub_out, og_job** job_out);

// ---- deposit ----------------------------------------------------------------------------------------------------------------------
int deposit_shape_query(uint64_t out[3]);                                                                                            // witness.hip
int deposit_records_ok(og_ctx* ctx, const uint8_t* inputs_d, size_t n, size_t base);
int deposit_witness(og_ctx* ctx, const uint8_t* inputs_d, size_t n, uint8_t* out_d);
int deposit_prove_batch(og_ctx* ctx, const og_pk* pk, const uint8_t* inputs_d, size_t n, const uint8_t* rs, uint8_t* proofs,       // groth16.hip
                        uint8_t* pub_out);

// ---- the record statements ----------------------------------------------------------------------------------------------------------
// where a statement's wires lie at a depth (a statement fills the landmarks its launches use)
struct RecordShape {
  uint64_t n_wires, n_constraints, first_bit_wire, first_gadget_wire, note_gadget_wires;
};

struct R1csBuilder;  // keygen.hip

struct RecordStatement {
  const char* name;                // "split" | "join" | "transfer": every message is formed from it
  int n_pub, n_rec, paths;         // public inputs; fields of a record before the siblings; sibling blocks per record (join: 2)
  const char* const* field_names;  // n_rec names
  const char* invalid_tail;        // how the boundary message ends: what, beyond ">= r", makes a field of this statement invalid
  int w9_xch;                      // exchange slots of the wave-wide walk per request, beyond one per level and path
  RecordShape (*shape)(int depth);
  // launches only, on ctx->stream; the caller asks hipGetLastError
  void (*launch_check)(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint32_t* bad_d);  // bad_d[g] = lowest offending field (atomicMin)
  void (*launch_core)(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d);  // the lane-local walk, Montgomery wires
  void (*launch_w9)(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint32_t* wl, uint32_t* xch);  // the wave-wide walk: three launches
  void (*r1cs_rows)(R1csBuilder& b, int depth);  // keygen.hip: the statement's wire table and rows
};
extern const RecordStatement ST_SPLIT, ST_JOIN, ST_TRANSFER;  // witness.hip

// bytes of one input record: the ONE place the width of a record is computed
inline size_t record_bytes(const RecordStatement& st, int depth) { return (size_t)(st.n_rec + st.paths * depth) * 32; }

void split_r1cs_rows(R1csBuilder& b, int depth);  // keygen.hip
void join_r1cs_rows(R1csBuilder& b, int depth);
void transfer_r1cs_rows(R1csBuilder& b, int depth);

// does a witness call of n requests walk wave-wide (k_w9_* and its kin)?  OG_WITNESS_W9 = 0 | 1 forces either way, OG_WITNESS_W9_MAX
// moves the bound (hooks builds only); otherwise calls of at most 512 requests do, a sub-batch of a larger call does not
bool witness_walks_wave_wide(const og_ctx* ctx, size_t n);                                                                              // witness.hip
int records_shape_query(const RecordStatement& st, int depth, uint64_t out[3]);  // n_wires | n_constraints | n_pub
// OG_ERR_INVALID names the first malformed record and its lowest offending field (`base` = index of record 0 in the caller's batch); blocking
int records_ok(const RecordStatement& st, og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, size_t base);
// records (checked: records_ok) -> n x n_wires x 32 B canonical, by the walk witness_walks_wave_wide picks
int records_witness(const RecordStatement& st, og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* out_d);
int records_prove_batch(const RecordStatement& st, og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n,        // groth16.hip
                        const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out);

}  // namespace og
