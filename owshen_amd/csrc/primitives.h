// What the leaf units offer to the entry points (capi.hip): the MiMC7 hash and tree (mimc7.hip), the field operations (field_ops.hip),
// the micro-benchmarks (ubench.hip), EdDSA verification (eddsa.hip), EdDSA keys and signing (eddsa_keys.hip) and stealth notes (notes.hip).
#pragma once
#include "ctx.h"

namespace og {

// ---- mimc7.hip ----------------------------------------------------------------------------------------------------------------------
int mimc7_init(og_ctx* ctx);
int mimc7_hash2(og_ctx* ctx, const uint8_t* l, const uint8_t* r, uint8_t* out, size_t n);
int mimc7_merkle_paths(og_ctx* ctx, const uint8_t* leaves, const uint64_t* idx, const uint8_t* sib, int depth,
                       uint8_t* nodes, size_t n);
int mimc7_tree_build(og_ctx* ctx, const uint8_t* leaves, size_t n, uint8_t* nodes);
int mimc7_append(og_ctx* ctx, int depth, const uint8_t* frontier_in, uint64_t next_index, const uint8_t* leaves, size_t k,
                 uint8_t* frontier_out, uint8_t* root_out);

// ---- field_ops.hip ------------------------------------------------------------------------------------------------------------------
int field_op(og_ctx* ctx, int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
int field_mulchain(og_ctx* ctx, int field, uint8_t* x, const uint8_t* y, size_t n, int iters, float* ms);
// form 0: lane-local fe_mul, one lane per element (64-lane workgroups); form 1: w9, one wave per element
int field_mulchain_lat(og_ctx* ctx, int field, int form, uint8_t* x, const uint8_t* y, size_t n, int iters, float* ms, uint64_t* cycles_out);

// ---- ubench.hip ---------------------------------------------------------------------------------------------------------------------
int ubench(og_ctx* ctx, int kind, int iters, int blocks, float* ms, uint64_t* wave_cycles);
// out[0] = resident kernel ms, out[1] = filler ms while the resident kernel runs (queued `delay_us` after it), out[2] = the
// same filler launch alone
int ubench_coresidency(og_ctx* ctx, int wgs_per_cu, int kind, int iters, int filler_blocks, int filler_threads, int filler_lds,
                       int filler_prio, int filler_work, int delay_us, float out[3]);

// ---- eddsa.hip ----------------------------------------------------------------------------------------------------------------------
int eddsa_verify(og_ctx* ctx, const uint8_t* recs_d, size_t n, uint32_t* ok_d);

// ---- eddsa_keys.hip -----------------------------------------------------------------------------------------------------------------
// pk_d (n x 64) and pkc_d (n x 32) may each be null
int eddsa_pubkey(og_ctx* ctx, const uint8_t* sk_d, size_t n, uint8_t* pk_d, uint8_t* pkc_d, uint32_t* ok_d);
// item i: the compressed key at in_d + i in_stride -> x | y at out_d + i out_stride, followed by a copy of the in_stride - 32 bytes
// behind the key (og_eddsa_verify_compressed_batch_d widens its 160-byte records to the 192 bytes eddsa_verify reads)
int eddsa_decompress(og_ctx* ctx, const uint8_t* in_d, size_t in_stride, size_t n, uint8_t* out_d, size_t out_stride, uint32_t* ok_d);
int eddsa_sign(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* records_d, uint32_t* ok_d);
// the 64 x 16 window table of BASE that ed_mul_base (eddsa.hip.h) walks: built on the context's stream by the first call, kept in ctx
int eddsa_base_table(og_ctx* ctx, const uint8_t** tab);

// ---- notes.hip ----------------------------------------------------------------------------------------------------------------------
// requests n x 160 B -> memos n x 160 B and notes n x 64 B
int note_seal(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d);
bool note_sk_canonical(const uint8_t sk[32]);
// sk: HOST, canonical (the caller has checked it); leaves_d (n x 32) and opened_d (n x 128) may each be null
int note_scan(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d, uint32_t* hit_d);
// the owned form (a note bound to a one-time key, spent by the claim statement): the same argument lists
int note_seal_owned(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d);
int note_scan_owned(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d, uint32_t* hit_d);
// the view form (find and open with the view scalar v and the public spend key PS, spend with sk): requests n x 224 B -> memos and
// notes as above; v, ps and sk: HOST, checked by the caller (note_ps_refusal: null, or why PS cannot be an address's spend key);
// rows_d and unlocked_d n x 128 B
int note_seal_view(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d);
const char* note_ps_refusal(const uint8_t ps[64]);
int note_scan_view(og_ctx* ctx, const uint8_t v[32], const uint8_t ps[64], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d,
                   uint32_t* hit_d);
int note_unlock(og_ctx* ctx, const uint8_t sk[32], const uint8_t* rows_d, const uint8_t* leaves_d, size_t n, uint8_t* unlocked_d, uint32_t* ok_d);

}  // namespace og
