// The statements between their translation units: what witness.hip (kernels, boundary checks, witness launches), keygen.hip (the R1CS
// builders), groth16.hip (records -> proofs) and capi.hip (the entry points) call of one another, declared once.
//
// withdraw, deposit, split, join, transfer, claim, send and redeem are one descriptor each: a record of n_rec fields and `paths` blocks of `depth` siblings
// (deposit: no path, and no depth), a shape that depends on StatementArgs, a boundary check, and one way from checked records to
// witnesses.  Everything that does not depend on the statement is written once over the descriptor ("adding a statement").
// split, join, transfer, claim, send and redeem -- the "record statements" -- share their witness entry too (records_witness: a
// lane-local walk for batches and a wave-wide one for small calls; the owned statements claim, send and redeem have no wave-wide form,
// their launch_w9 is NULL and every call walks lane-local) and their R1CS prologue and epilogue; the four members at the end of the
// descriptor are theirs, and NULL / 0 for withdraw and deposit: only records_witness and keygen.hip's records_r1cs_build read them, and
// only those six statements are routed there.
#pragma once
#include "ctx.h"
#include "msm.hip.h"  // arena_get

namespace og {

// what a statement's shape depends on: the depth of the tree (deposit: none) and withdraw's padding gates (every other statement: 0)
struct StatementArgs {
  int depth;
  uint64_t n_pad3, n_pad2;
};

// where a statement's wires lie (a statement fills the landmarks its launches use)
struct RecordShape {
  uint64_t n_wires, n_constraints, first_bit_wire, first_gadget_wire, note_gadget_wires;
};

struct R1csBuilder;  // keygen.hip

struct Statement {
  const char* name;                // "withdraw" | "deposit" | "split" | "join" | "transfer" | "claim" | "send" | "redeem": every message is formed from it
  int n_pub, n_rec, paths;         // public inputs; fields of a record before the siblings; sibling blocks per record (deposit: 0, join: 2)
  const char* const* field_names;  // n_rec names
  const char* invalid_tail;        // how the boundary message ends, after the field's name: what makes a field of this statement invalid
  const char* key_noun;            // what a key of another shape "is not for"
  RecordShape (*shape)(const StatementArgs& a);
  // a launch only, on ctx->stream; the caller asks hipGetLastError.  bad_d[g] = lowest offending field of record g (atomicMin)
  void (*launch_check)(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d);
  // records (checked) -> n x n_wires x 32 B canonical, enqueued on ctx->stream
  int (*witness)(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint8_t* out_d);
  // ---- the record statements only
  int w9_xch;  // exchange slots of the wave-wide walk per request, beyond one per level and path
  void (*launch_core)(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d);  // the lane-local walk, Montgomery wires
  // the wave-wide walk: three launches.  NULL: the statement has none, and records_witness walks lane-local whatever n
  void (*launch_w9)(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint32_t* wl, uint32_t* xch);
  void (*r1cs_rows)(R1csBuilder& b, int depth);  // keygen.hip: the statement's wire table and rows
};
extern const Statement ST_WITHDRAW, ST_DEPOSIT, ST_SPLIT, ST_JOIN, ST_TRANSFER, ST_CLAIM, ST_SEND, ST_REDEEM;  // witness.hip

// bytes of one input record: the ONE place the width of a record is computed
inline size_t record_bytes(const Statement& st, int depth) { return (size_t)(st.n_rec + st.paths * depth) * 32; }

void split_r1cs_rows(R1csBuilder& b, int depth);  // keygen.hip
void join_r1cs_rows(R1csBuilder& b, int depth);
void transfer_r1cs_rows(R1csBuilder& b, int depth);
void claim_r1cs_rows(R1csBuilder& b, int depth);
void send_r1cs_rows(R1csBuilder& b, int depth);
void redeem_r1cs_rows(R1csBuilder& b, int depth);

// does a witness call of n requests walk wave-wide (k_w9_* and its kin)?  OG_WITNESS_W9 = 0 | 1 forces either way, OG_WITNESS_W9_MAX
// moves the bound (hooks builds only); otherwise calls of at most 512 requests do, a sub-batch of a larger call does not
bool witness_walks_wave_wide(const og_ctx* ctx, size_t n);                                                                              // witness.hip
int records_shape_query(const Statement& st, const StatementArgs& a, uint64_t out[3]);  // n_wires | n_constraints | n_pub
// the boundary check of n records, enqueued: the argument checks and the statement's launch (bad_d: n words of 0xff before it runs)
int records_check_enqueue(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d);
// "<who>: input record <g>: field <f> (<its name>) <the statement's tail>": the message of a flag records_check_enqueue left
std::string invalid_record_message(const Statement& st, const std::string& who, int depth, size_t g, uint32_t f);
// OG_ERR_INVALID names the first malformed record and its lowest offending field (`base` = index of record 0 in the caller's batch); blocking
int records_ok(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, size_t base);
// the witness entry of split, join, transfer, claim, send and redeem: the walk witness_walks_wave_wide picks, where the statement has both
int records_witness(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint8_t* out_d);

// records -> proofs, slab by slab: check, witnesses, the batched prover                                                               // groth16.hip
int statement_prove_batch(const Statement& st, og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n,
                          const uint8_t* rs, uint8_t* proofs, uint8_t* pub_out);
// withdraw alone may generate its witnesses inside the prover's pipeline, and has an enqueue-only and a window-sharded form
int withdraw_prove_batch(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                         uint8_t* proofs, uint8_t* pub_out);
int withdraw_prove_batch_submit(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                                uint8_t* proofs, uint8_t* pub_out, og_job** job_out);
int withdraw_prove_partials_enqueue(og_ctx* ctx, const og_pk* pk, const StatementArgs& a, const uint8_t* inputs_d, size_t n, int win_rank,
                                    int win_world, uint8_t* partials_d, uint8_t* pub_out, og_job** job_out);

}  // namespace og
