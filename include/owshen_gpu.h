/* owshen_gpu.h -- C ABI of libowshen_gpu.so, the MI355X (gfx950) Groth16 prover path.
 *
 * Drop-in boundary.  The reference snapshot has NO FFI seam and NO
 * prover, so none of these entry points *replaces* an existing
 * extern; each one cites the reference call site it is shaped to serve:
 *
 *   - proof generation would be called from `withdraw_handler`
 *     (/root/reference/src/services/api_services/withdraw.rs:27-71, between the
 *     ECDSA recover at :34 and the sequencer re-sign at :56);
 *   - proof verification would gate `burn_tx`
 *     (/root/reference/src/blockchain/tx/burn_tx.rs:11-32, before the balance debit);
 *   - every field element crossing this boundary uses the byte format of the
 *     reference's `Fp::to_repr()`: 32 bytes, little-endian, canonical (< modulus)
 *     (/root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:7-11);
 *   - errors follow the callers' `anyhow::Result` convention
 *     (/root/reference/src/utils.rs:5-20): 0 = ok, negative = error, message via
 *     og_last_error(); nothing unwinds across the boundary.
 *
 * Conventions
 *   Fr / Fq element : 32 B little-endian canonical.
 *   G1 affine       : x || y (64 B); the point at infinity is 64 zero bytes.
 *   G2 affine       : x.c0 || x.c1 || y.c0 || y.c1 (128 B); infinity = 128 zero bytes.
 *   proof           : A(G1) || B(G2) || C(G1) = 256 B.
 *   "_d" pointers are DEVICE pointers (HBM, e.g. from og_malloc or a torch tensor's
 *   data_ptr()); all other pointers are host memory owned by the caller; the library
 *   never retains a caller pointer past return.  One og_ctx per GPU (one process per
 *   GPU); calls on one ctx are blocking and internally serialised.
 *   Randomness is never drawn inside the library: (r, s) are explicit inputs.
 */
#ifndef OWSHEN_GPU_H
#define OWSHEN_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_ctx og_ctx;
typedef struct og_bases og_bases; /* device-resident, Montgomery-form MSM bases */
typedef struct og_pk og_pk;       /* device-resident proving key + R1CS matrices */

#define OG_OK 0
#define OG_ERR_INVALID (-1)  /* bad argument / malformed input */
#define OG_ERR_HIP (-2)      /* HIP runtime failure (message has the hipError string) */
#define OG_ERR_NO_DEVICE (-3)
#define OG_ERR_UNSATISFIED (-4) /* witness does not satisfy the circuit: some row has a*b != c, or wire 0 != 1 (exact) */

/* ---- lifecycle ---------------------------------------------------------- */
int og_init(int device, og_ctx** out);
void og_shutdown(og_ctx* ctx);
const char* og_last_error(void); /* thread-local, valid until the next failing call */
int og_device_count(void);
int og_sync(og_ctx* ctx);
/* the HIP stream every kernel of this ctx is launched on (hipStream_t as void*) */
void* og_stream(og_ctx* ctx);

/* ---- device memory plumbing --------------------------------------------- */
int og_malloc(og_ctx* ctx, size_t bytes, void** out_d);
int og_free(og_ctx* ctx, void* ptr_d);
int og_memcpy_h2d(og_ctx* ctx, void* dst_d, const void* src, size_t bytes);
int og_memcpy_d2h(og_ctx* ctx, void* dst, const void* src_d, size_t bytes);

/* ---- N1: field arithmetic (test / micro-bench surface) --------------------
 * op: 0 add, 1 sub, 2 mul, 3 inv(a) (b ignored; inv(0) = 0).  field: 0 = Fr, 1 = Fq. */
int og_field_op_d(og_ctx* ctx, int field, int op, const uint8_t* a_d, const uint8_t* b_d,
                  uint8_t* out_d, size_t n);
/* chained Montgomery multiplications: x <- x*y repeated `iters` times per element;
 * returns kernel milliseconds (HIP events on the ctx stream) in *ms_out. */
int og_field_mulchain_d(og_ctx* ctx, int field, uint8_t* x_d, const uint8_t* y_d, size_t n,
                        int iters, float* ms_out);

/* the same chain as a LATENCY probe: form 0 = the lane-local product, one lane per element (64-lane workgroups); form 1 = the
 * wave-wide "w9" product (csrc/field_w9.hip.h: one element over nine lanes of a wave, ~80 instead of 205 instructions per
 * product), one wave per element, n <= 65535.  Same bytes out as og_field_mulchain_d.  *wave_cycles_out (may be NULL) = the
 * longest wave's loop in shader cycles. */
int og_field_mulchain_lat_d(og_ctx* ctx, int field, int form, uint8_t* x_d, const uint8_t* y_d, size_t n,
                            int iters, float* ms_out, uint64_t* wave_cycles_out);

/* VALU instruction-rate probe: every lane runs iters x 16 independent instructions.
 * kind: 0 v_mad_u64_u32, 1 v_mul_lo_u32, 2 v_mul_hi_u32, 3 v_add_co_u32, 4 v_addc_co_u32,
 * 5 v_lshl_add_u64, 6 v_add_u32, 7 v_mad_u32_u24, 8 v_mul_hi_u32_u24, 9 v_mov_b32.
 * blocks x 256 lanes.  Kernel milliseconds in *ms_out. */
int og_ubench(og_ctx* ctx, int kind, int iters, int blocks, float* ms_out);
/* same, plus kinds 10 v_fma_f64 and 11 v_add_f64; *wave_cycles_out = the longest wave's loop time in SHADER CYCLES
 * (s_memtime): with all waves resident, cycles / (iters x 16 x waves per SIMD) is the issue cost per wave-instruction
 * with no clock assumption, and cycles / ms the effective clock of the run.
 * Further kinds probe what the column-serial field products rely on: 12 one dependent v_mad_u64_u32 chain,
 * 13 v_lshrrev_b64, 14 the chain with an s_nop after every instruction, 15 / 16 two / four interleaved chains, 17 the chain
 * with vcc as the carry-out destination, 20 + k: k interleaved chains, 40 + k: the same ping-ponging between two register
 * pairs, 100 + 5 a + b: one chain on v[40:41] with its factors in VGPR banks a and b (b = 4: second factor in an SGPR);
 * 202: `iters` wave-wide MiMC7 rounds on a lone wave (blocks x 64 lanes; mimc7.hip.h w9_mimc7_round: two rows of the wave, the
 * 32-bit Montgomery digit -- what the launches use; 200 / 201, the one-row form and the 29-bit digit, in the hooks build only):
 * *wave_cycles_out / iters = cycles per round. */
int og_ubench_cycles(og_ctx* ctx, int kind, int iters, int blocks, float* ms_out, uint64_t* wave_cycles_out);
/* co-residency probe (what a short kernel on a second stream gets done beside a persistent kernel that holds `wgs_per_cu`
 * one-wave, 128-register workgroups on every CU): kind 0 = the resident waves run a dependent v_mad_u64_u32 chain, 1 = they
 * sleep.  out[0] = resident kernel ms, out[1] = filler ms beside it (queued delay_us later), out[2] = the filler alone. */
int og_ubench_coresidency(og_ctx* ctx, int wgs_per_cu, int kind, int iters, int filler_blocks, int filler_threads,
                          int filler_lds, int filler_prio, int filler_work, int delay_us, float out[3]);

/* ---- N5: MiMC7 (circomlib convention, 91 rounds) -------------------------- */
/* the 91 round constants, canonical LE, for cross-checking against the oracle */
int og_mimc7_constants(og_ctx* ctx, uint8_t out[91 * 32]);
/* out[i] = MultiMiMC7([left[i], right[i]], key = 0) */
int og_mimc7_hash2_d(og_ctx* ctx, const uint8_t* left_d, const uint8_t* right_d, uint8_t* out_d,
                     size_t n);
/* n paths of `depth` levels.  index bit l = 1 => node at level l is a right child.
 * siblings: n x depth x 32 B.  nodes_out: n x (depth+1) x 32 B (leaf first, root last). */
int og_mimc7_merkle_paths_d(og_ctx* ctx, const uint8_t* leaves_d, const uint64_t* indices_d,
                            const uint8_t* siblings_d, int depth, uint8_t* nodes_out_d, size_t n);
/* full tree over n = 2^k leaves.  nodes_out: (2n-1) x 32 B in level order:
 * [leaves (n) | level 1 (n/2) | ... | root (1)]. */
int og_mimc7_tree_build_d(og_ctx* ctx, const uint8_t* leaves_d, size_t n, uint8_t* nodes_out_d);
/* Batched append to an append-only depth-`depth` tree kept as a frontier (the "filled subtrees" of deposit contracts;
 * empty leaves are 0) -- the commitment tree `mint_tx` (/root/reference/src/blockchain/tx/mint_tx.rs:11-49) would feed,
 * SURVEY.md 8f-3.  frontier_*_d: depth x 32 B (must not alias); next_index = leaves already in the tree; k >= 1 new
 * leaves; root_out_d: 32 B.  Level by level on the GPU: ~k hashes in total, `depth` launches.  Frontier entries at
 * levels where bit l of (next_index + k) is 0 are unspecified: an append never reads them before rewriting them. */
int og_mimc7_append_d(og_ctx* ctx, int depth, const uint8_t* frontier_in_d, uint64_t next_index, const uint8_t* leaves_d,
                      size_t k, uint8_t* frontier_out_d, uint8_t* root_out_d);

/* ---- airdrop signatures: batched EdDSA verification on BabyJubJub with the MiMC7 sponge ----------
 * The reference's `PointCompressed::verify` (/root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:99-115)
 * with its placeholder product hash (:202-204) replaced by MultiMiMC7: accepts iff pk and R lie on the curve and
 *   s * BASE == R + h * pk,   h = MultiMiMC7([R.x, R.y, pk.x, pk.y, message], key 0).
 * records_d: n records of 6 x 32 B canonical LE: pk.x | pk.y | R.x | R.y | s | message (public keys affine; for compressed
 * keys, mod.rs:88-98, see og_eddsa_verify_compressed_batch_d below).  ok_out: HOST, n x u32 (1 accept / 0 reject; a
 * non-canonical field element rejects). */
int og_eddsa_verify_batch_d(og_ctx* ctx, const uint8_t* records_d, size_t n, uint32_t* ok_out);

/* ---- airdrop keys: compressed keys, key derivation and signing on the GPU -------------------------------------------
 * The rest of the reference's BabyJubJub surface: `PrivateKey::to_pub` (mod.rs:207-209), `PrivateKey::sign` (:210-236, hash :=
 * MultiMiMC7 as above) and the decompression inside `PointCompressed::verify` (:88-98).  One item per lane; device pointers in,
 * ok_out a HOST array of n x u32; n = 0 is OG_OK; a null handle or pointer is OG_ERR_INVALID before the device is touched.
 *
 * Compressed key, 32 B: x canonical LE with the parity of y (`is_odd` of the canonical integer, mod.rs:82-84) in bit 255
 * (0x80 of byte 31).  Bit 254 must be clear and x < r, otherwise the key is refused.  The reference's `PointCompressed(Fp, bool)`
 * has no packed form: this one is this library's (it is NOT circomlib's packing, which stores y with the sign of x).
 *
 * og_eddsa_pubkey_batch_d: pk = sk * BASE as x | y (pk_out_d, n x 64 B) and / or compressed (pkc_out_d, n x 32 B); either output
 *   may be NULL.  ok = 0 and zeroed outputs for a non-canonical sk; sk = 0 and sk = l (the order of BASE) give the identity (0, 1).
 * og_eddsa_decompress_batch_d: y = sqrt((1 - a x^2) / (1 - d x^2)), negated when its parity differs from the flag; y = 0 is
 *   returned for either flag.  ok = 0 and 64 zero bytes when the encoding is refused or the value has no square root (the
 *   reference's "Cannot take sqrt": about half of all x).
 * og_eddsa_sign_batch_d: requests of 3 x 32 B: sk | randomness | message.  r = MultiMiMC7([randomness, message]), R = r * BASE,
 *   pk = sk * BASE, h = MultiMiMC7([R.x, R.y, pk.x, pk.y, message]), s = (r + h * sk) mod ORDER (ORDER = 8 l).  records_out_d:
 *   n complete records of og_eddsa_verify_batch_d (6 x 32 B), so signing and verification chain on the device.  ok = 0 and a
 *   zeroed record for a non-canonical input, and when s >= r (the reference's "Invalid repr").
 * og_eddsa_verify_compressed_batch_d: records of 5 x 32 B: compressed pk | R.x | R.y | s | message.  ok = 1 iff the key
 *   decompresses and og_eddsa_verify_batch_d accepts the record with the decompressed key; everything else is 0 (where the
 *   reference returns Err: a refused encoding, a key without a square root, a non-canonical field). */
int og_eddsa_pubkey_batch_d(og_ctx* ctx, const uint8_t* sk_d, size_t n, uint8_t* pk_out_d, uint8_t* pkc_out_d, uint32_t* ok_out);
int og_eddsa_decompress_batch_d(og_ctx* ctx, const uint8_t* pkc_d, size_t n, uint8_t* pk_out_d, uint32_t* ok_out);
int og_eddsa_sign_batch_d(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* records_out_d, uint32_t* ok_out);
int og_eddsa_verify_compressed_batch_d(og_ctx* ctx, const uint8_t* records_d, size_t n, uint32_t* ok_out);

/* ---- stealth notes: seal a note to a public key, scan the pool's memos on the GPU ------------------------------------
 * What connects the keys above to the pool's statements: a sender pays a payee it knows only by its public key, with no round
 * trip, and the payee's wallet finds and opens its notes by scanning every memo the pool has published.  With H = MultiMiMC7
 * 2-to-1 (key 0), BASE and `multiply` as in the reference's babyjubjub/mod.rs (:68-78, :177-188), l the order of BASE, and
 * small(P) <=> 8 P = (0, 1):
 *   keys    sk: any canonical Fr element; pk = sk * BASE (og_eddsa_pubkey_batch_d).
 *   KDF     from a shared point S (affine): k = H(S.x, S.y); tag = H(k, 1); nullifier' = H(k, 2); secret' = H(k, 3);
 *           pad_a = H(k, 4); pad_t = H(k, 5).
 *   seal    request, 5 x 32 B: e | pk.x | pk.y | amount | token.  E = e * BASE, S = e * pk, c' = H(nullifier', secret'),
 *           leaf = H(c', H(amount, token)) -- the leaf shape of every statement.
 *           memo, 5 x 32 B: E.x | E.y | tag | amount + pad_a mod r | token + pad_t mod r  (what a ledger publishes beside the leaf);
 *           note, 2 x 32 B: c' | leaf  (c' is the `pay_commitment` of og_transfer_prove_batch_d, leaf its `pay_leaf`).
 *           Refused (ok = 0, memo and note zeroed): a field >= r, amount >= 2^128, pk off the curve, small(pk), small(E)
 *           (that is, e = 0 mod l).
 *   scan    per memo S = sk * E, then the KDF.  hit = 0: a field >= r, E off the curve, small(E), or another tag -- memos come from
 *           anybody, so a malformed memo is never an error of the call; hit = 2: the tag is this key's and the memo does not
 *           open (the decrypted amount is >= 2^128, or leaves were given and the recomputed leaf differs): hostile or broken,
 *           to be ignored; hit = 1: the payee's, opened as nullifier' | secret' | amount | token (4 x 32 B) -- what a withdraw /
 *           split / join / transfer record of the leaf's index spends.  small(E) is refused because E = (0, 1) would give every
 *           wallet the same S.  sk is NOT reduced mod l: E may carry torsion, and S is `multiply` on the integer sk < r.
 * Every field 32 B little-endian canonical.  Device pointers in; ok_out / hit_out are HOST arrays of n x u32; n = 0 is OG_OK with no
 * pointer needed; a null handle or required pointer is OG_ERR_INVALID before the device is touched.
 * og_note_scan_batch_d: sk is a HOST pointer (OG_ERR_INVALID for sk >= r); leaves_d (n x 32 B, the published leaf beside each memo)
 *   and opened_out_d (n x 4 x 32 B) may each be NULL; rows of opened_out_d are zero unless the hit is 1.  The scalar is the same
 *   for all n memos: it is recoded once on the host and neither sk nor its digits stay in the context after the call. */
int og_note_seal_batch_d(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_out_d, uint8_t* notes_out_d, uint32_t* ok_out);
int og_note_scan_batch_d(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_out_d, uint32_t* hit_out);

/* ---- owned notes: a note sealed to a ONE-TIME key, which only the payee can spend ----------------------------------------------------
 * The notes above have a hole.  Their spending secrets nullifier' = H(k, 2) and secret' = H(k, 3) derive from S = e * pk = sk * E, and
 * the SENDER chose e: the sender knows S, k and both secrets, every statement spends a note on knowledge of (nullifier, secret) alone,
 * so whoever pays such a note can spend it again before the payee does, and can watch for its nullifier hash.  The owned form is the
 * usual fix for stealth addresses: the note is bound to a one-time public key P = pk + t * BASE.  The sender can compute P; only
 * the payee knows its discrete logarithm x = sk + t mod l, and the claim statement (og_claim_prove_batch_d, below) spends the note
 * on knowledge of x.  Notation as above, l = ORDER / 8 the prime order of BASE:
 *   KDF     from S, on indices disjoint from 1..5: k = H(S.x, S.y); tag = H(k, 6); t = H(k, 7); pad_a = H(k, 8); pad_t = H(k, 9).
 *           Because the indices are disjoint, og_note_scan_batch_d answers 0 for an owned memo and og_note_scan_owned_batch_d
 *           answers 0 for an ordinary one.
 *   seal    request as above.  E = e * BASE, S = e * pk, P = pk + t * BASE, c = H(P.x, P.y), leaf = H(c, H(amount, token)) -- the
 *           pool's leaf shape with c in the commitment's place.  memo: E.x | E.y | tag | amount + pad_a | token + pad_t; note: c | leaf.
 *           Refused: what og_note_seal_batch_d refuses, and small(P).
 *   scan    S = sk * E, then the KDF.  hit 0 and hit 2 as above; hit 1 opens the memo as x | amount | token | c (4 x 32 B) with
 *           x = (sk + t) mod l, written canonically, and c = H(P.x, P.y) for P = x * BASE -- with the leaf's index and siblings, the
 *           private half of a claim record.  When leaves are given, each is compared with H(c, H(amount, token)); a difference is
 *           hit 2.  Only a lane whose tag matches computes t, x, P, c and the leaf.  The host passes sk mod l beside the recoded
 *           digits, as a kernel argument: neither sk nor anything derived from it stays in the context.
 * Two facts: a sender who reuses e for the same pk makes two notes with one x, of which only one can be claimed (one nullifier
 * hash) -- the loss is the sender's; a pk with a torsion component can never be claimed (P = pk + t * BASE is then outside the
 * subgroup x * BASE generates) -- the fault lies with the key's owner.  The specification is tests/owned_note_spec.py.
 * Arguments, sizes and refusals of the calls: those of og_note_seal_batch_d and og_note_scan_batch_d. */
int og_note_seal_owned_batch_d(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_out_d, uint8_t* notes_out_d, uint32_t* ok_out);
int og_note_scan_owned_batch_d(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_out_d, uint32_t* hit_out);

/* ---- view keys: find and open owned notes without the key that spends them -------------------------------------------------------------
 * og_note_scan_owned_batch_d takes sk, the wallet's only secret: whoever scans can spend.  A scan is a service by nature (a machine
 * that is not the wallet walks the whole pool), so the view form separates the two powers, as every deployed stealth-address scheme
 * does.  Notation as above.
 *   keys    a view scalar v and a spend scalar sk, both canonical Fr elements; PV = v * BASE, PS = sk * BASE; the address is (PV, PS),
 *           which og_eddsa_pubkey_batch_d makes from [v, sk].
 *   KDF     from S, on indices disjoint from 1..5 and 6..9: k = H(S.x, S.y); tag = H(k, 10); t = H(k, 11); pad_a = H(k, 12);
 *           pad_t = H(k, 13).  Each of the three scans answers 0 on the memos of the other two forms.
 *   seal    request, 7 x 32 B: e | PV.x | PV.y | PS.x | PS.y | amount | token.  E = e * BASE, S = e * PV, P = PS + t * BASE,
 *           c = H(P.x, P.y), leaf = H(c, H(amount, token)).  memo, 5 x 32 B: E.x | E.y | tag | amount + pad_a | token + pad_t; note,
 *           2 x 32 B: c | leaf -- both the owned form's shapes, so a ledger stores them alike.  Refused (ok = 0, outputs zeroed): a
 *           field >= r, amount >= 2^128, PV or PS off the curve, small(PV), small(PS), small(E), small(P).
 *   scan    with (v, PS): S = v * E on the integer v < r (not reduced mod l), then the KDF.  hit 0: a field >= r, E off the curve,
 *           small(E), or another tag; hit 2: the tag matches and the amount is >= 2^128, or small(P), or leaves were given and the
 *           leaf differs from H(c, H(amount, token)); hit 1: the memo opens as t | amount | token | c (4 x 32 B), t the KDF's output,
 *           canonical and not reduced, c = H(P.x, P.y) for P = PS + t * BASE.  No x appears anywhere: the scanner never holds sk.
 *   unlock  with sk, in the wallet: row t | amount | token | c -> x | amount | token | c with x = (sk + t) mod l -- byte for byte the
 *           opened row of og_note_scan_owned_batch_d, the private half of a claim record.  ok = 1 only if the four fields are
 *           canonical, amount < 2^128, H(x * BASE) = c and, when leaves are given, leaf = H(c, H(amount, token)); otherwise ok = 0
 *           and the row is zeroed.  The all-zero row a scan writes for a non-hit gives ok = 0 by itself.
 * What each party knows: the sender t and P, not x.  The view-key holder t, P, amount, token and c; not x and not the nullifier hash
 * H(x, 1): it finds and reads notes, it cannot spend them and cannot see them spent.  The tag depends on v alone: two addresses with
 * one view key and different spend keys open each other's memos with a c that is not the sealed one -- hit 2 with a leaf; without a
 * leaf the scan cannot tell, and unlock with a leaf can.  A PS with a torsion component seals, and the note never unlocks
 * (x * BASE != P).  A scanning service may withhold notes, or lie about amount and token: unlock with the leaf catches the lie,
 * nothing catches withholding.  The specification is tests/view_note_spec.py.
 * Conventions of the owned pair: v, ps (PS.x | PS.y) and sk are HOST pointers; ok_out / hit_out are HOST arrays; leaves_d and
 * opened_out_d may be NULL; n = 0 is OG_OK and touches nothing; a null handle or required pointer is OG_ERR_INVALID before the device
 * is touched.  OG_ERR_INVALID, naming the reason, also for v >= r, sk >= r, and a PS with a coordinate >= r, off the curve or small
 * (decided once per call, on the host).  Neither v, sk, their digits nor sk mod l stay in the context. */
int og_note_seal_view_batch_d(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_out_d, uint8_t* notes_out_d, uint32_t* ok_out);
int og_note_scan_view_batch_d(og_ctx* ctx, const uint8_t v[32], const uint8_t ps[64], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_out_d, uint32_t* hit_out);
int og_note_unlock_batch_d(og_ctx* ctx, const uint8_t sk[32], const uint8_t* rows_d, const uint8_t* leaves_d, size_t n, uint8_t* unlocked_out_d, uint32_t* ok_out);

/* ---- N4: radix-2 Fr NTT(domain generator 7^((r-1)/n), coset generator 7) ------
 * batch transforms of size n = 2^log_n, natural order in and out, canonical bytes.
 *   inverse = 0, coset = 0 : out[i] = sum_j in[j] w^(ij)
 *   inverse = 0, coset = 1 : evaluates at 7 w^i
 *   inverse = 1            : the inverse maps (including the 1/n and 7^-j factors)
 * in_d and out_d must not overlap. */
int og_ntt_fr_d(og_ctx* ctx, const uint8_t* in_d, uint8_t* out_d, int log_n, int batch, int inverse,
                int coset);
/* Groth16 quotient: h = (A*B - C)/Z from the evaluations of A, B, C over the size-2^log_d
 * domain (3 iNTT, 3 coset NTT, pointwise, 1 coset iNTT).  batch x d x 32 B each; h_out_d gets
 * the d coefficients of h (coefficient d-1 is 0 for a satisfied R1CS). */
int og_h_poly_d(og_ctx* ctx, const uint8_t* a_d, const uint8_t* b_d, const uint8_t* c_d, int log_d,
                int batch, uint8_t* h_out_d);

/* ---- N2/N3: Pippenger MSM over G1 / G2 -------------------------------------
 * Bases are imported once (canonical affine -> device-resident Montgomery tables) and reused
 * by every MSM over them -- the shape of a Groth16 proving key, which is fixed across proofs.
 *   group        : 1 = G1 (64 B points), 2 = G2 (128 B points)
 *   window_bits  : 8, 12 or 16 (15 or 17 with precompute); 0 = choose from n
 *   precompute   : 1 = also store 2^(c k) P_i for every window k (nwin x the memory, one bucket
 *                  set instead of nwin: faster for repeated MSMs); 0 = plain
 * Points are NOT checked for curve membership (the key comes from a trusted setup). */
int og_bases_create_d(og_ctx* ctx, int group, const uint8_t* points_d, size_t n, int window_bits,
                      int precompute, og_bases** out);
void og_bases_free(og_bases* bases);
/* `batch` independent MSMs over the same bases: result[g] = sum_i s[g][i] * P_i, i < n.
 * scalars_d: batch vectors of n x 32 B, vector g starting at scalars_d + g * stride_bytes.
 * n may be smaller than the number of bases unless the bases were created with precompute.
 * out: HOST buffer, batch x (64 | 128) B canonical affine (zeros = point at infinity). */
int og_msm_d(og_ctx* ctx, const og_bases* bases, const uint8_t* scalars_d, size_t n, int batch,
             size_t stride_bytes, uint8_t* out);

/* Window-sharded MSM across GPUs (BASELINE.json configs[3]): bases replicated on every rank, scalars
 * broadcast, rank `win_rank` of `win_world` accumulates only the windows k with k % win_world == win_rank.
 *   og_msm_windows_d  this rank's share -> partial_out_d: og_msm_partial_slots(bases) points in the library's internal
 *                     extended form (128 B each in G1, 256 B in G2; opaque, only og_msm_combine_d reads them): one per
 *                     window for plain bases (infinity for windows the rank does not own), ONE partial sum for
 *                     precomputed tables.  n must equal the number of bases for precomputed tables.
 *   (all-gather of the ranks' partial arrays: <= 16 x 256 B per rank -- an RCCL all-gather, never an all-reduce: curve
 *    points do not add limb-wise.  owshen_amd/shard.py does it with torch.distributed, og_multi_* inside the library.)
 *   og_msm_combine_d  gathered_d: world x slots points, rank-major -> sum over ranks per slot, Horner over the windows;
 *                     out: HOST, 64 | 128 B canonical affine. */
int og_msm_partial_slots(const og_bases* bases);
int og_msm_windows_d(og_ctx* ctx, const og_bases* bases, const uint8_t* scalars_d, size_t n, int win_rank, int win_world,
                     uint8_t* partial_out_d);
int og_msm_combine_d(og_ctx* ctx, const og_bases* bases, const uint8_t* gathered_d, int world, uint8_t* out);

/* ---- N6: Groth16 proving -----------------------------------------------------
 * The proving key is parsed once and stays resident in HBM (R1CS matrices in CSR, the five query
 * vectors as precomputed window tables).  Serialized key, little-endian, every section padded to
 * a multiple of 32 B:
 *   u64 x 10 : "OWPK0001", n_wires, n_pub, log_d, n_rows, nnz_a, nnz_b, nnz_c, flags, 0
 *              (flags bit 0: no C matrix -- nnz_c = 0 -- and C z := (A z) o (B z): a key that og_zkey_import made)
 *   alpha_g1 | beta_g1 | delta_g1 | 64 B pad | beta_g2 | delta_g2
 *   for M in A, B, C: row_ptr (n_rows+1 u32) | col (nnz u32) | val (nnz x 32 B)
 *   a_query (m) | b_g1_query (m) | b_g2_query (m, G2) | l_query (m - n_pub - 1) | h_query (d - 1)
 * Rows = the constraints followed by the n_pub + 1 input-consistency rows (A = wire i, B = C = 0);
 * d = 2^log_d >= n_rows.  Wire 0 is the constant 1, wires 1..n_pub are public.
 * A witness is n_wires x 32 B; (r, s) are the caller's blinding scalars, r || s (64 B), explicit so that
 * a proof is a pure function of (key, witness, r, s).  A proof is A (G1) || B (G2) || C (G1) = 256 B.
 * OG_ERR_UNSATISFIED: a witness does not satisfy the R1CS (og_last_error names the first one).  The check is exact: every
 * QAP row product a_i b_i = c_i is tested and wire 0 must be the constant 1, so OG_OK means every returned proof verifies.
 * OG_ERR_INVALID: a witness holds a value that is not the canonical encoding of an Fr element (>= r); og_last_error names
 * the witness and its first such wire.  Checked on the GPU for every caller-supplied witness (one more read of it), before
 * "does not satisfy": the reference's `Fp::from_repr` rejects such bytes
 * (/root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:7-11), and reducing them silently would prove a
 * statement about a different byte string than the caller holds.
 * The blinding scalars are NOT under that rule: r and s are any 32-byte values, read as integers below 2^256 and used modulo the
 * group order, so the proof for (r, s) is byte for byte the proof for (r mod order, s mod order) -- they are randomness the caller
 * chose, not part of a statement, and a reduced value proves nothing different.  Every form of the assembly keeps this (the
 * kernels walk all 256 bits and reduce r s in the field layer; a call that holds one such scalar forms none of its products from
 * GLV halves, since og_glv_decompose refuses a non-canonical scalar): tests/assembly_edge_cases.py pins it for r, s in
 * {order, order + 7, 2^256 - 1}. */
int og_pk_load(og_ctx* ctx, const uint8_t* blob, size_t len, og_pk** out);
/* Frees the key's device memory.  Waits for the device first, so a submitted call that still reads the key finishes its
 * kernels -- but its results are only delivered by og_job_wait, which the caller still owes (or og_job_abandon). */
void og_pk_free(og_pk* pk);
/* info[0..3] = n_wires, n_pub, log_d, n_rows */
int og_pk_info(const og_pk* pk, uint64_t info[4]);
/* Query density: a wire whose base is the point at infinity in a query (the wire never occurs in that matrix) is dropped
 * from that query's table and digit sort -- except that queries whose wire lists coincide up to a few wires share one list
 * (and one digit sort per sub-batch); the few bases a query lacks stay in its table as points at infinity and are skipped.
 * out[0..3] = points actually accumulated per proof by the A query (G1), the B query (once in G1 and once in G2), the L
 * query (G1) and the H query (G1, d - 1). */
int og_pk_density(const og_pk* pk, uint64_t out[4]);
/* Window bits of the A, B, L and H queries' precomputed tables: a query of n points costs n x ceil(255 / bits) bucket
 * additions per proof (16 bits from 8 k points on, 17 bits from 160 k points on: owshen_amd/csrc/msm.hip). */
int og_pk_windows(const og_pk* pk, uint64_t out[4]);
/* The row-basis extension, "OWPR0001": key material BESIDE an OWPK0001 blob (the blob itself never changes), little-endian:
 *   u64 x 4 : "OWPR0001", n_rows, log_d, 0
 *   32 B    : Keccak-256 of the OWPK0001 blob it belongs to
 *   [L_j(tau)]_1 for j < n_rows (64 B each) | [L_j(tau)]_2 for j < n_rows (128 B each), canonical affine
 * L_j: the Lagrange basis of the key's domain.  With a_i(x) = sum_j A[j,i] L_j(x), sum_i z_i [a_i(tau)] = sum_j (A z)_j [L_j(tau)]
 * -- the same group element, so the same proof bytes -- and the prover already has A z and B z for the quotient.  With the
 * extension og_pk_load_rows decides per query, at load: the A query (and, once for its G1 and G2 copies, the B query) runs
 * over the rows with an entry in its matrix when   rows x windows(rows) <= 0.8 x wires x windows(wires)
 * (additions against additions; near-ties stay on the wires).  The L and H queries never change.  A key whose A / B queries
 * hold clearly more wire bases than its matrices have non-empty rows gains; every other key loads exactly as og_pk_load
 * loads it.  rows == NULL / rows_len == 0: og_pk_load.
 * A wrong extension is refused, OG_ERR_INVALID, og_last_error naming the cause: its length or header, a digest that is not
 * this blob's, and -- for an extension that will be used -- a coordinate >= q, a point off its curve, or points that do not
 * reproduce the blob's own queries (one multi-scalar multiplication in each form per query and group, over a vector derived
 * from the digest).  Uses the context's scratch: OG_ERR_INVALID while a submitted call is in flight.
 *   og_setup_rows     og_setup, and the key's extension in *rows_out (malloc'd; og_blob_free) -- or NULL / 0 when the rule
 *                     would keep both queries of this circuit on the wires.  og_setup_ptau and og_zkey_import make none.
 *   og_pk_query_form  what the five queries A | B (G1) | B (G2) | L | H run, four words each: form (OG_QUERY_FORM_*), points
 *                     (entries of its digit sort = points of its table), window bits, table (queries with the same number
 *                     share one set of window tables: A and B (G1) in row form).  og_pk_density and og_pk_windows keep
 *                     describing the blob's wire queries.
 * The evaluation form of the quotient is decided at load too, by og_pk_load and og_pk_load_rows alike and from the blob alone: a
 * key that has a C matrix and a domain of 2^14 or more keeps h on the coset -- its H tables hold the DFT of the H query (d
 * points), its L tables L_i + [the fold of C's column i] over the L wires and every other wire of C -- so that a proof takes
 * four transforms instead of seven.  The same group elements, the same proof bytes; a derived table that does not reproduce the
 * blob's own L and H queries fails the load, OG_ERR_INVALID.  Such a key reports OG_QUERY_FORM_EVAL for L and H.  That
 * load-time check uses the context's scratch, as og_pk_load_rows' does: for a key that takes this form og_pk_load and
 * og_pk_load_rows answer OG_ERR_INVALID while a submitted call is in flight (og_job_wait it first); a key that stays in
 * the coefficient form loads through og_pk_load beside a pending job as before. */
#define OG_QUERY_FORM_WIRE 0 /* over the wires (H: over the quotient's coefficients) */
#define OG_QUERY_FORM_ROW 1  /* A, B: over the QAP rows */
#define OG_QUERY_FORM_EVAL 2 /* L, H: H over the coset values of (A z)(B z), C z folded into L */
int og_pk_load_rows(og_ctx* ctx, const uint8_t* blob, size_t len, const uint8_t* rows, size_t rows_len, og_pk** out);
int og_pk_query_form(const og_pk* pk, uint64_t out[20]);
/* Witnesses in HOST memory (n x n_wires x 32 B; pageable is fine): each sub-batch is copied to the device inside the
 * prover's stage pipeline, under the accumulations of the sub-batch before it -- measured 510 proofs/s against 519 with
 * the same 2^18-wire witnesses already resident (og_prove_batch_d), 8.4 MB per proof over PCIe. */
int og_prove(og_ctx* ctx, const og_pk* pk, const uint8_t* witness, const uint8_t rs[64], uint8_t proof_out[256]);
int og_prove_batch(og_ctx* ctx, const og_pk* pk, const uint8_t* witnesses, size_t n, const uint8_t* rs,
                   uint8_t* proofs_out);
/* same, witnesses already resident in HBM (n x n_wires x 32 B); rs and proofs_out are host buffers */
int og_prove_batch_d(og_ctx* ctx, const og_pk* pk, const uint8_t* witnesses_d, size_t n, const uint8_t* rs,
                     uint8_t* proofs_out);

/* ---- multi-GPU from ONE process -----------------------------------------------------
 * The reference node is a single process with one Context (/root/reference/src/cli/node.rs:71-76), so the library itself
 * drives every GPU of the node: one og_ctx per device, one host thread per device per call, RCCL (ncclCommInitAll) for the
 * one exchange step that exists.  Handle arrays (og_pk**, og_bases**) have og_multi_size() entries, one per device.
 *   og_multi_init          n_devices = 0: every visible device.  Fails if fewer are visible than asked for.
 *   og_multi_prove_batch   proofs sharded across the devices in contiguous slices (key replicated, NO data-path collective:
 *   og_multi_withdraw_...  proofs are independent units); same bytes as the single-device calls.  All buffers are HOST.
 *   og_multi_msm           one MSM window-sharded over the devices (BASELINE.json configs[3] names this sharding): scalars
 *                          (host) -> device 0 -> ncclBroadcast over xGMI; rank g accumulates the windows k = g (mod G);
 *                          ncclAllGather of the per-window points (<= 16 x 256 B per rank; an all-gather, not an all-reduce:
 *                          curve points do not add limb-wise); Horner combine.  out: host, 64 | 128 B canonical affine. */
typedef struct og_multi og_multi;
int og_multi_init(int n_devices, og_multi** out);
void og_multi_shutdown(og_multi* m);
int og_multi_size(const og_multi* m);
/* out[0], out[1] = the contiguous slice [lo, hi) of a batch of n proofs that device `rank` proves (og_multi_prove_batch /
 * og_multi_withdraw_prove_batch): sizes differ by at most one, the first n mod G devices take the larger ones, a device whose
 * slice is empty sits the call out.  BASELINE.json configs[3] (4096 proofs over 8 GPUs) = 512 each. */
int og_multi_slice(const og_multi* m, size_t n, int rank, size_t out[2]);
og_ctx* og_multi_ctx(og_multi* m, int rank);
/* out[0] = the HIP device ordinal rank `rank` is bound to; pci_out = that device's PCI address ("0000:5d:00.0"); when the
 * devices share an RCCL communicator (more than one device): out[1] = ncclCommCount, out[2] = ncclCommUserRank, out[3] =
 * ncclCommCuDevice of this rank's communicator, else zeros.  A bench line quotes these so that "N ranks on N GPUs" is a
 * reading of the runtime, not a claim. */
int og_multi_device_info(const og_multi* m, int rank, uint64_t out[4], char pci_out[32]);
int og_multi_pk_load(og_multi* m, const uint8_t* blob, size_t len, og_pk** pks_out);
void og_multi_pk_free(og_multi* m, og_pk** pks);
int og_multi_prove_batch(og_multi* m, og_pk* const* pks, const uint8_t* witnesses, size_t n, const uint8_t* rs,
                         uint8_t* proofs_out);
/* public_out (host, may be NULL): n x 6 x 32 B, as og_withdraw_prove_batch_d */
int og_multi_withdraw_prove_batch(og_multi* m, og_pk* const* pks, int depth, uint64_t n_pad3, uint64_t n_pad2,
                                  const uint8_t* inputs, size_t n, const uint8_t* rs, uint8_t* proofs_out,
                                  uint8_t* public_out);
/* Window-sharded PROVING (BASELINE.json north_star: "MSM windows shard naturally across GPUs"; configs[3] as written): ONE
 * batch of n proofs on all N devices together -- every device generates the n witnesses and quotients itself (replicated:
 * they are latency chains / a few per cent of a proof), sorts and accumulates only the windows k = rank (mod N) of all five
 * queries over the replicated key, the per-proof partial points (768 B per proof and rank) are exchanged with ONE
 * ncclAllGather over xGMI -- never an all-reduce: curve points do not add limb-wise -- and device 0 adds the shares and
 * assembles the proofs.  Same arguments, same bytes out, same errors as og_multi_withdraw_prove_batch / og_multi_prove_batch
 * (which shard by PROOFS and stay the throughput form: a proof-sharded batch does no work twice); this form cuts the latency
 * of one request or a handful, the case of the one-request-per-call site
 * /root/reference/src/services/api_services/withdraw.rs:27-71.  N <= 15 (one rank per 17-bit window at most). */
int og_multi_withdraw_prove_sharded(og_multi* m, og_pk* const* pks, int depth, uint64_t n_pad3, uint64_t n_pad2,
                                    const uint8_t* inputs, size_t n, const uint8_t* rs, uint8_t* proofs_out,
                                    uint8_t* public_out);
int og_multi_prove_sharded(og_multi* m, og_pk* const* pks, const uint8_t* witnesses, size_t n, const uint8_t* rs,
                           uint8_t* proofs_out);
int og_multi_bases_create(og_multi* m, int group, const uint8_t* points, size_t n, int window_bits, int precompute,
                          og_bases** bases_out);
void og_multi_bases_free(og_multi* m, og_bases** bases);
int og_multi_msm(og_multi* m, og_bases* const* bases, const uint8_t* scalars, size_t n, uint8_t* out);

/* ---- N6: Groth16 verification (CPU only: no og_ctx, no GPU -- the `burn_tx` seam,
 * /root/reference/src/blockchain/tx/burn_tx.rs:11-32, must work on a sequencer without one) ----------
 * Evaluates the EIP-197 predicate e(-A,B) e(alpha,beta) e(IC_0 + sum x_i IC_i, gamma) e(C,delta) == 1.
 * vk: "OWVK0001" | u64 n_pub | alpha_g1 (64) | beta_g2 (128) | gamma_g2 (128) | delta_g2 (128) | IC ((n_pub+1) x 64).
 * public_inputs: n_pub x 32 B.  *ok_out = 1 accept / 0 reject; a proof with a non-canonical coordinate, a point
 * off the curve or outside the r-torsion, or a public input >= r is a REJECT (ok = 0, OG_OK), a malformed key
 * is OG_ERR_INVALID. */
int og_verify(const uint8_t* vk, size_t vk_len, const uint8_t* public_inputs, size_t n_pub,
              const uint8_t proof[256], int* ok_out);

/* ---- N6 on the GPU: batched Groth16 verification behind a key handle ----------------------------------------------------
 * og_vk_load decodes and subgroup-checks an "OWVK0001" key ONCE and keeps on the device everything that depends on the key
 * alone: the Miller value of (alpha, beta), the whole twist walk of gamma and of delta (slope and intercept of each of the 102
 * steps of the optimal-ate loop) and 4-bit fixed-base window tables of the IC points (60 KB per public input).  A key that
 * makes og_verify answer OG_ERR_INVALID (magic, length, n_pub, an invalid alpha / beta / gamma / delta / IC point) makes
 * og_vk_load answer OG_ERR_INVALID.  og_vk_info: info = { n_pub, steps of the stored walks, bytes of IC tables, device bytes }.
 * The handle belongs to the DEVICE it was loaded on and may be freed before or after og_shutdown of the loading context.
 *
 * og_verify_batch_d checks n proofs in one call, one proof per GPU lane: public_inputs_d is n x n_pub x 32 B and proofs_d
 * n x 256 B, both DEVICE pointers (16-byte aligned, as og_malloc returns); ok_out is a HOST array of n u32, 1 accept / 0 reject.
 * The number of public inputs is the key's -- a count that differs from the key's cannot be expressed.  ok_out[i] is what
 * og_verify(vk, public_inputs[i], n_pub, proofs[i]) answers, for every input: a non-canonical coordinate, a point off the
 * curve, B outside the r-torsion, A, B or C at infinity, or a public input >= r (tested before the infinite-IC shortcut) is a
 * REJECT (ok = 0, OG_OK); when vk_x is the point at infinity its pairing is skipped.  n = 0 is OG_OK.  Null handles are
 * OG_ERR_INVALID before the device is touched.  No randomness is drawn: every proof gets its own pairing check (the final
 * exponentiation is a structured chain that raises og_verify's value to a fixed power prime to r -- the same decision).
 * og_verify itself, and libowshen_verify.so, are unchanged: the host-only verifier is what a sequencer without a GPU uses. */
typedef struct og_vk og_vk; /* device-resident verifying key + everything that depends on the key alone */
int og_vk_load(og_ctx* ctx, const uint8_t* vk, size_t vk_len, og_vk** out);
void og_vk_free(og_vk* vk);
int og_vk_info(const og_vk* vk, uint64_t info[4]);
int og_verify_batch_d(og_ctx* ctx, const og_vk* vk, const uint8_t* public_inputs_d, const uint8_t* proofs_d, size_t n,
                      uint32_t* ok_out);

/* ---- withdraw circuit: batched witness generation (N5 feeding N6) ----------------------------
 * The statement (public: root, nullifier_hash, recipient, amount, token, chain_id; private: nullifier, secret and a
 * depth-`depth` MiMC7 Merkle path; leaf = H(H(nullifier, secret), H(amount, token))) and its wire order are specified in
 * oracle/py/withdraw.py and built as an R1CS by og_withdraw_r1cs / owshen_amd/circuit.py.  The six public inputs cover
 * what the reference's gate signs (/root/reference/contracts/src/Owshen.sol:69: msg.sender, token, amount, id, chainid;
 * nullifier_hash stands in for the replay id).  n_pad3 / n_pad2 append synthetic multiplication gates
 * that size the statement (BASELINE.json: "MSM ~2^20 G1 points, Fr NTT 2^17"); 0 / 0 is the natural circuit.
 * inputs_d: n records of (8 + depth) x 32 B:
 *   nullifier | secret | amount | recipient | pad_seed | index (u64, low bytes) | token | chain_id | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  shape[0..2] = n_wires, n_constraints, n_pub. */
int og_withdraw_shape(int depth, uint64_t n_pad3, uint64_t n_pad2, uint64_t shape[3]);
int og_withdraw_witness_d(og_ctx* ctx, int depth, uint64_t n_pad3, uint64_t n_pad2, const uint8_t* inputs_d,
                          size_t n, uint8_t* witness_out_d);
/* input records -> proofs in one call (what `withdraw_handler` wants): every sub-batch's witnesses are generated by
 * the lane that proves them, in lane-private scratch, so the full n x n_wires witness array never exists and the
 * latency-bound MiMC7 walk overlaps the other lane's MSMs.  Same bytes as og_withdraw_witness_d + og_prove_batch_d.
 * pk must be a key for this (depth, n_pad3, n_pad2) shape.  rs: n x 64 B host, proofs_out: n x 256 B host.
 * public_out (host, may be NULL): n x 6 x 32 B, every proof's public inputs in verifier order (root, nullifier_hash,
 * recipient, amount, token, chain_id) -- root and nullifier_hash are COMPUTED by the witness generator, so the caller
 * needs them back to submit the proof.
 * OG_ERR_INVALID: an input record is malformed -- a field >= r (two encodings would map to one nullifier), or an index that
 * does not fit the tree (>= 2^depth, or bytes above the u64 set); og_last_error names the record and its first such field
 * (0 nullifier, 1 secret, 2 amount, 3 recipient, 4 pad_seed, 5 index, 6 token, 7 chain_id, 8 + l sibling l).  The records
 * arrive from HTTP (/root/reference/src/services/api_services/withdraw.rs:15-19); og_withdraw_witness_d checks the same. */
int og_withdraw_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2,
                              const uint8_t* inputs_d, size_t n, const uint8_t* rs, uint8_t* proofs_out,
                              uint8_t* public_out);

/* ---- deposit statement (BASELINE.json north_star: "deposit/withdraw circuits") ---------------------------------------------
 * public: commitment, depositor; private: nullifier, secret; commitment = H(nullifier, secret) (MultiMiMC7), depositor bound by
 * its square (oracle/py/deposit.py is the spec; 735 wires, 731 constraints, domain 2^10).  The reference's deposit credits an
 * account on the word of an L1 transaction hash (/root/reference/src/services/api_services/deposit.rs:32-154 ->
 * /root/reference/src/blockchain/tx/mint_tx.rs:11-49: no commitment, no proof); with notes, the ledger forms the leaf
 * H(c, H(amount, token)) from the depositor's c and the asset it credits -- and this proof lets it refuse a c nobody can open
 * (a typo, a c copied from somebody else's request), i.e. a note that could never be withdrawn.  The ledger's side is og_verify
 * with public inputs (c, depositor = DepositRequest.address, deposit.rs:19-24).
 * inputs_d: n records of 3 x 32 B: nullifier | secret | depositor.  shape[0..2] = n_wires, n_constraints, n_pub.
 * og_deposit_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host, public_out (host, may be NULL):
 * n x 2 x 32 B = commitment | depositor per proof).  Errors as og_withdraw_prove_batch_d (a field >= r: OG_ERR_INVALID naming
 * the record and its field 0 nullifier, 1 secret, 2 depositor). */
int og_deposit_shape(uint64_t shape[3]);
int og_deposit_witness_d(og_ctx* ctx, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_deposit_prove_batch_d(og_ctx* ctx, const og_pk* pk, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                             uint8_t* proofs_out, uint8_t* public_out);

/* ---- split statement: withdraw part of a note, keep the rest as a fresh change note ----------------------------------------------
 * "I know a note under `root` worth `amount` of `token`.  I take `amount_out` of it out to `recipient`.  The rest, change =
 * amount - amount_out, goes into the new leaf `change_leaf`."  (No reference counterpart: the snapshot's withdraw burns a whole
 * amount, /root/reference/src/services/api_services/withdraw.rs:27-71.)
 * public (n_pub = 7, verifier order): root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf
 * private: nullifier, secret, amount, change_commitment, change, a depth-`depth` MiMC7 Merkle path.  With H = MultiMiMC7 2-to-1:
 *   leaf = H(H(nullifier, secret), H(amount, token)) is under root at `index`;  nullifier_hash = H(nullifier, 0);
 *   amount_out + change = amount with amount_out < 2^128 and change < 2^128 (a 128-bit decomposition each: the sum stays below
 *   2^129 < r and cannot wrap -- this is what stops an overdraw);
 *   change_leaf = H(change_commitment, H(change, token)) -- the leaf shape of a deposit, so the change note is later spent by the
 *   withdraw or the split statement like any other;  recipient and chain_id are bound by a square each.
 * `amount` is PRIVATE here: only amount_out is revealed, not the size of the note that was spent.  change_commitment is an
 * unconstrained private input, c' = H(nullifier', secret') formed by the prover off-circuit (a c' nobody can open harms only
 * the prover: the argument of the deposit statement).  amount_out = 0 with somebody else's c' is a transfer inside the pool;
 * amount_out = amount leaves a zero-value change note.  The ledger's part: og_verify the proof, check that root is known and
 * nullifier_hash unspent, pay amount_out, append change_leaf (og_mimc7_append_d).
 * Wire and row order: tests/split_spec.py (the spec), og_split_r1cs / owshen_amd/circuit.py split_r1cs (the R1CS):
 *   n_wires = 271 + 3 depth + (6 + depth) 730 - 3, n_constraints = 261 + 2 depth + (6 + depth) 730 (28 104 / 28 065 at depth
 *   32: domain 2^15).  depth 1..64; n <= 65 535 per og_split_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (9 + depth) x 32 B canonical little-endian:
 *   nullifier | secret | amount | recipient | amount_out | index (u64, low bytes) | token | chain_id | change_commitment | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  og_split_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 7 x 32 B in verifier order -- root, nullifier_hash and change_leaf are COMPUTED by the
 * witness generator).  Same bytes as og_split_witness_d + og_prove_batch_d.  The key must have this shape's wire count and n_pub.
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 4 (amount_out)"; 0 nullifier, 1 secret, 2 amount, 3 recipient, 4 amount_out, 5 index, 6 token,
 * 7 chain_id, 8 change_commitment, 9 + l sibling l): any field >= r; an index that does not fit the tree; field 2 if amount >=
 * 2^128; field 4 if amount_out >= 2^128 or amount_out > amount (compared as integers).
 * The witness generator has two walks with the same bytes: one lane per request for batches, and for calls of at most 512 requests
 * the wave-wide form of the withdraw statement -- a permutation per wave in three launches, the four permutations of the change
 * note beside the dependent chain, which is as long as withdraw's.  There is no submit / job form, no multi-GPU form and no
 * window-sharded form of this statement, and og_set_host_chains does not change how its witnesses are generated. */
int og_split_shape(int depth, uint64_t shape[3]);
int og_split_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_split_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                           uint8_t* proofs_out, uint8_t* public_out);

/* ---- join statement: merge two notes into one (the inverse of split) ---------------------------------------------------------------
 * "I know two different notes under `root`, worth `amount_a` and `amount_b` of the same token.  Both are spent.  Their sum goes
 * into the new leaf `out_leaf`."  Nothing leaves the pool.  (No reference counterpart: the snapshot has no circuit.)
 * public (n_pub = 5, verifier order): root, nullifier_hash_a, nullifier_hash_b, chain_id, out_leaf
 * private: per note nullifier, secret, amount and a depth-`depth` MiMC7 Merkle path; token (ONE wire shared by all three asset
 * hashes; private because nothing is paid out); out_commitment; sum; nh_diff_inv.  With H = MultiMiMC7 2-to-1, for x in {a, b}:
 *   leaf_x = H(H(nullifier_x, secret_x), H(amount_x, token)) is under root at `index_x`;  nullifier_hash_x = H(nullifier_x, 0);
 *   the last level of BOTH walks has the root wire as its output -- that is what says "the same root", there is no equality row;
 *   amount_a + amount_b = sum with amount_a, amount_b and sum each < 2^128 (a 128-bit decomposition each: the two input checks
 *   keep the sum below 2^129 < r whatever a ledger appended, the check on sum keeps the new note spendable by split);
 *   (nullifier_hash_a - nullifier_hash_b) nh_diff_inv = 1 -- the same note counted twice is unprovable, whatever the order in
 *   which a ledger marks nullifiers;  out_leaf = H(out_commitment, H(sum, token)), the leaf shape of a deposit;  chain_id is bound
 *   by its square.
 * out_commitment is an unconstrained private input, c' = H(nullifier', secret') formed off-circuit, as in split.  The ledger's
 * part, in order: og_verify the proof, check that root is known, check that BOTH nullifier hashes are unspent, mark both, append
 * out_leaf (og_mimc7_append_d).
 * Wire and row order: tests/join_spec.py (the spec), og_join_r1cs / owshen_amd/circuit.py join_r1cs (the R1CS):
 *   n_wires = 396 + 6 depth + (10 + 2 depth) 730, n_constraints = 390 + 4 depth + (10 + 2 depth) 730 (54 608 / 54 538 at depth 32:
 *   74 hashes, domain 2^16).  depth 1..64; n <= 65 535 per og_join_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (11 + 2 depth) x 32 B canonical little-endian:
 *   nullifier_a | secret_a | amount_a | index_a (u64, low bytes) | nullifier_b | secret_b | amount_b | index_b | token | chain_id
 *   | out_commitment | siblings_a[depth] | siblings_b[depth]
 * witness_out_d: n x n_wires x 32 B.  og_join_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 5 x 32 B in verifier order -- root, both nullifier hashes and out_leaf are COMPUTED by the
 * witness generator).  Same bytes as og_join_witness_d + og_prove_batch_d.  The key must have this shape's wire count and n_pub.
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 6 (amount_b)"; 0 nullifier_a, 1 secret_a, 2 amount_a, 3 index_a, 4 nullifier_b, 5 secret_b, 6 amount_b,
 * 7 index_b, 8 token, 9 chain_id, 10 out_commitment, 11 + l sibling a of level l, 11 + depth + l sibling b of level l): any
 * field >= r; an index that does not fit the tree (3 or 7); field 2 if amount_a >= 2^128; field 6 if amount_b >= 2^128 or
 * amount_a + amount_b >= 2^128 (compared as integers); field 4 if nullifier_b == nullifier_a (nh_diff_inv would not exist).
 * Two notes whose walks end in DIFFERENT roots cannot be seen at that boundary: og_join_witness_d fills the root wire from note
 * a's walk, and og_join_prove_batch_d answers OG_ERR_UNSATISFIED through the prover's row check.
 * The witness generator has two walks with the same bytes.  For batches every request gets two lanes, one per note, through one
 * rolled permutation body.  For calls of at most 512 requests it is the wave-wide form of the withdraw statement -- a permutation
 * per wave in three launches, the two notes' chains side by side (each as long as withdraw's), the joined note's four permutations
 * and nh_diff_inv beside them; there too the root wire is note a's alone.  Out of scope for this statement: the lane-pair round
 * (t^4 beside t^3), the wave-per-request walk and host chains (og_set_host_chains does not change how its witnesses are
 * generated); there is no submit / job form, no multi-GPU form and no window-sharded form of the call. */
int og_join_shape(int depth, uint64_t shape[3]);
int og_join_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_join_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                          uint8_t* proofs_out, uint8_t* public_out);

/* ---- transfer statement: pay part of a note to somebody else INSIDE the pool, keep the rest ---------------------------------------
 * "I know a note under `root` worth `amount` of `token`.  It is spent.  `pay_amount` of it goes into the new leaf `pay_leaf`.  The
 * rest, change = amount - pay_amount, goes into the new leaf `change_leaf`."  Nothing leaves the pool.  With it the set closes: any
 * in-pool payment is zero or more joins followed by one transfer.  (No reference counterpart: the snapshot has no circuit.)
 * public (n_pub = 5, verifier order): root, nullifier_hash, chain_id, pay_leaf, change_leaf
 * private: nullifier, secret, amount, token, pay_commitment, pay_amount, change_commitment, change, a depth-`depth` MiMC7 Merkle path.
 * `token` is ONE wire shared by all three asset hashes, private as in join: nothing is paid out.  With H = MultiMiMC7 2-to-1:
 *   leaf = H(H(nullifier, secret), H(amount, token)) is under root at `index`;  nullifier_hash = H(nullifier, 0);
 *   pay_amount + change = amount with pay_amount < 2^128 and change < 2^128 (a 128-bit decomposition each: the sum stays below
 *   2^129 < r and cannot wrap -- this is what makes it impossible to create value);
 *   pay_leaf = H(pay_commitment, H(pay_amount, token));  change_leaf = H(change_commitment, H(change, token)) -- both have the leaf
 *   shape of a deposit, so either note is later spent by withdraw, split, join or transfer like any other;  chain_id is bound by
 *   its square.
 * pay_commitment and change_commitment are unconstrained private inputs, each a c' = H(nullifier', secret') formed off-circuit; the
 * payee hands over the first one (a c' nobody can open harms only the prover: the argument of the split statement).
 * pay_amount = 0 and pay_amount = amount are both allowed.  The ledger's part: og_verify the proof, check that root is known and
 * nullifier_hash unspent (and mark it), append pay_leaf, then change_leaf (og_mimc7_append_d).
 * Wire and row order: tests/transfer_spec.py (the spec), og_transfer_r1cs / owshen_amd/circuit.py transfer_r1cs (the R1CS):
 *   n_wires = 267 + 3 depth + (8 + depth) 730, n_constraints = 260 + 2 depth + (8 + depth) 730 (29 563 / 29 524 at depth 32:
 *   domain 2^15).  depth 1..64; n <= 65 535 per og_transfer_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (9 + depth) x 32 B canonical little-endian:
 *   nullifier | secret | amount | index (u64, low bytes) | token | chain_id | pay_commitment | pay_amount | change_commitment | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  og_transfer_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 5 x 32 B in verifier order -- root, nullifier_hash and both leaves are COMPUTED by the
 * witness generator).  Same bytes as og_transfer_witness_d + og_prove_batch_d.  The key must have this shape's wire count and n_pub.
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 7 (pay_amount)"; 0 nullifier, 1 secret, 2 amount, 3 index, 4 token, 5 chain_id, 6 pay_commitment,
 * 7 pay_amount, 8 change_commitment, 9 + l sibling l): any field >= r; an index that does not fit the tree; field 2 if amount >=
 * 2^128; field 7 if pay_amount >= 2^128 or pay_amount > amount (compared as integers).
 * The witness generator has two walks with the same bytes: one lane per request for batches, and for calls of at most 512 requests
 * the wave-wide form of the withdraw statement -- a permutation per wave in three launches, the eight permutations of the two
 * output notes beside the dependent chain, which is as long as withdraw's.  Out of scope for this statement: the lane-pair round
 * and the wave-per-request walk, host chains (og_set_host_chains does not change how its witnesses are generated), a submit / job
 * form, a multi-GPU form and a window-sharded form of the call, and Rust and Solidity bindings (ffi/ and contracts/ are frozen).
 * split and join take the same three launches for calls of the same size. */
int og_transfer_shape(int depth, uint64_t shape[3]);
int og_transfer_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_transfer_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                              uint8_t* proofs_out, uint8_t* public_out);

/* ---- claim statement: turn an owned note into an ordinary note of the same value that only the claimant can open ---------------------
 * "I know the discrete logarithm x of the one-time key P of an owned note under `root`.  It is spent.  Its whole value goes into the
 * new leaf `out_leaf`."  Nothing leaves the pool; after it withdraw, split, join and transfer work unchanged on the out note.  The
 * sender of the owned note knows pk, e, S, t and P but not x = sk + t: with any x' of their own, x' * BASE is another point, c another
 * value and the root the statement publishes is not the tree's.  (No reference counterpart: the snapshot has no circuit.)
 * public (n_pub = 4, verifier order): root, nullifier_hash, chain_id, out_leaf
 * private: x, amount, token, out_commitment, a depth-`depth` MiMC7 Merkle path.  With H = MultiMiMC7 2-to-1, l the order of BASE:
 *   x = sum 2^i b_i over 251 boolean wires (one recomposition row);
 *   x < l, against the constant m = l - 1, most significant bit first: t starts as 1; at a 1-bit of m a new wire t <- t b_i (one row);
 *     at a 0-bit of m the row b_i t = 0 (114 wires, 251 rows).  NOT optional: l has 251 bits and 2^251 - l ~ 0.32 l, so without it
 *     about a third of all keys have a second representation x + l with another nullifier_hash -- a double spend;
 *   P = x * BASE bit by bit: T_i = 2^i * BASE = (u_i, v_i) are constants, (x1, y1) is the running sum from (0, 1); per bit the rows
 *     b (b - 1) = 0, w1 = b x1, w2 = b y1, w3 = w1 y1, x3 (1 + d u_i v_i w3) = x1 + (v_i - 1) w1 + u_i w2,
 *     y3 (1 - d u_i v_i w3) = y1 + (v_i - 1) w2 - a u_i w1 -- the complete twisted Edwards law with the addend (b u_i, 1 + b (v_i - 1)),
 *     linear in the bit; no denominator can vanish (1 255 wires, 1 506 rows);
 *   c = H(P.x, P.y);  asset = H(amount, token);  leaf = H(c, asset) is under root at `index`;
 *   nullifier_hash = H(x, 1): an ordinary spend publishes H(nullifier, 0), so both kinds share the ledger's spent set and never collide;
 *   out_leaf = H(out_commitment, asset): the SAME asset wire, so value and token carry over without a range check;  chain_id is
 *   bound by its square.
 * out_commitment is an unconstrained private input, a c' = H(nullifier', secret') the claimant forms off-circuit.  The ledger's part:
 * og_verify the proof, check that root is known and nullifier_hash unspent (and mark it), append out_leaf (og_mimc7_append_d).
 * Wire and row order: tests/claim_spec.py (the spec), og_claim_r1cs / owshen_amd/circuit.py claim_r1cs (the R1CS):
 *   n_wires = 1627 + 3 depth + (5 + depth) 730, n_constraints = 3 + 1506 + 251 + 730 (5 + depth) + 2 depth (28 733 / 28 834 at depth 32:
 *   domain 2^15; the 3: chain_id^2, the recomposition of x, and one * one = one on the constant wire).  depth 1..64; n <= 65 535 per
 *   og_claim_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (6 + depth) x 32 B canonical little-endian:
 *   x | amount | token | chain_id | out_commitment | index (u64, low bytes) | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  og_claim_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 4 x 32 B in verifier order).  Same bytes as og_claim_witness_d + og_prove_batch_d.  The key must
 * have this shape's wire count and n_pub.
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 0 (x)"; 0 x, 1 amount, 2 token, 3 chain_id, 4 out_commitment, 5 index, 6 + l sibling l): any field >= r;
 * field 0 if x >= l; field 1 if amount >= 2^128; an index that does not fit the tree.
 * The witness generator has ONE walk, one lane per request whatever n: the 251 affine partial sums are walked projectively, parked
 * in their own wire slots and brought to affine by one inversion per request (Montgomery's trick).  Out of scope: a wave-wide walk,
 * host chains, a submit / job form, a multi-GPU and a window-sharded form, and Rust and Solidity bindings (ffi/ and contracts/ are
 * frozen). */
int og_claim_shape(int depth, uint64_t shape[3]);
int og_claim_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_claim_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                           uint8_t* proofs_out, uint8_t* public_out);

/* ---- send statement: an owned note pays part of itself to somebody else INSIDE the pool and keeps the rest -------------------------
 * "I know the discrete logarithm x of the one-time key P of an owned note under `root`, worth `amount` of `token`.  It is spent.
 * `pay_amount` of it goes into the new leaf `pay_leaf`, the rest into the new leaf `change_leaf`."  Nothing leaves the pool.  It is
 * transfer for an owned note: one proof where claim followed by transfer took two.  After it claim is needed only in front of join.
 * (No reference counterpart: the snapshot has no circuit.)
 * public (n_pub = 5, verifier order): root, nullifier_hash, chain_id, pay_leaf, change_leaf -- transfer's list
 * private: x, amount, token, pay_commitment, pay_amount, change_commitment, change, a depth-`depth` MiMC7 Merkle path.
 * The front is the claim statement's, gadget for gadget (above: the decomposition of x, x < l, P = x * BASE), without its
 * one * one = one row:
 *   x = sum 2^i b_i over 251 boolean wires;  x < l against l - 1 (114 wires, 251 rows);  P = x * BASE (1 255 wires, 1 506 rows);
 *   c = H(P.x, P.y);  asset = H(amount, token);  leaf = H(c, asset) is under root at `index`;
 *   nullifier_hash = H(x, 1).  claim, send and redeem publish the SAME nullifier_hash for the same note, so the ledger's one spent
 *     set stops a note that was claimed from also being sent or redeemed;
 * the back is the transfer statement's:
 *   pay_amount + change = amount with pay_amount < 2^128 and change < 2^128 (a 128-bit decomposition each: the sum cannot wrap);
 *   pay_leaf = H(pay_commitment, H(pay_amount, token));  change_leaf = H(change_commitment, H(change, token)), over the ONE token
 *   wire;  chain_id is bound by its square.
 * pay_commitment and change_commitment are unconstrained: each may be an ordinary c' = H(nullifier', secret') or the c of an owned or
 * view note (og_note_seal_owned_batch_d / og_note_seal_view_batch_d return it), which is what lets the payer seal the pay note to the
 * payee's address and the change note to its own.  pay_amount = 0 and pay_amount = amount are both allowed.
 * The ledger's part: og_verify the proof, check that root is known and nullifier_hash unspent (and mark it), append pay_leaf, then
 * change_leaf (og_mimc7_append_d).
 * Wire and row order: tests/send_spec.py (the spec), og_send_r1cs / owshen_amd/circuit.py send_r1cs (the R1CS):
 *   n_wires = 1886 + 3 depth + (8 + depth) 730, n_constraints = 2018 + 2 depth + (8 + depth) 730 (31 182 / 31 282 at depth 32:
 *   domain 2^15; the 2018: chain_id^2, the sum, 2 x 129 range rows, the recomposition of x, 251 + 1 506).  depth 1..64; n <= 65 535
 *   per og_send_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (8 + depth) x 32 B canonical little-endian:
 *   x | amount | token | chain_id | pay_commitment | pay_amount | change_commitment | index (u64, low bytes) | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  og_send_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 5 x 32 B in verifier order).  Same bytes as og_send_witness_d + og_prove_batch_d.  The key must
 * have this shape's wire count and n_pub (a transfer key has the n_pub and is refused by its wire count).
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 5 (pay_amount)"; 0 x, 1 amount, 2 token, 3 chain_id, 4 pay_commitment, 5 pay_amount, 6 change_commitment,
 * 7 index, 8 + l sibling l): any field >= r; field 0 if x >= l; field 1 if amount >= 2^128; field 5 if pay_amount >= 2^128 or
 * pay_amount > amount (compared as integers); field 7 if the index does not fit the tree.
 * The witness generator has ONE walk, one lane per request whatever n: the claim statement's walk of x * BASE, then the hashes.
 * Out of scope: a wave-wide walk, host chains, a submit / job form, a multi-GPU and a window-sharded form, and Rust and Solidity
 * bindings (ffi/ and contracts/ are frozen). */
int og_send_shape(int depth, uint64_t shape[3]);
int og_send_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_send_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                          uint8_t* proofs_out, uint8_t* public_out);

/* ---- redeem statement: an owned note pays part of itself OUT of the pool to a recipient and keeps the rest --------------------------
 * "I know the discrete logarithm x of the one-time key P of an owned note under `root`.  It is spent.  I take `amount_out` of it out
 * to `recipient`, and the rest goes into the new leaf `change_leaf`."  It is split for an owned note: one proof where claim followed
 * by split took two.  (No reference counterpart: the snapshot has no circuit.)
 * public (n_pub = 7, verifier order): root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf -- split's list
 * private: x, amount, change_commitment, change, a depth-`depth` MiMC7 Merkle path.  `amount` stays private.
 * The front is the claim statement's, as in the send statement (no one * one = one row):
 *   x = sum 2^i b_i over 251 boolean wires;  x < l;  P = x * BASE;  c = H(P.x, P.y);  asset = H(amount, token);  leaf = H(c, asset) is
 *   under root at `index`;  nullifier_hash = H(x, 1) -- the SAME nullifier_hash claim and send publish for the note: one spent set;
 * the back is the split statement's:
 *   amount_out + change = amount with amount_out < 2^128 and change < 2^128 (a 128-bit decomposition each);
 *   change_leaf = H(change_commitment, H(change, token));  recipient and chain_id are bound by a square each.
 * change_commitment is unconstrained: an ordinary c' or the c of an owned or view note.  amount_out = 0 and amount_out = amount are both
 * allowed.  The ledger's part: og_verify the proof, check that root is known and nullifier_hash unspent (and mark it), pay amount_out of
 * token to recipient, append change_leaf (og_mimc7_append_d).
 * Wire and row order: tests/redeem_spec.py (the spec), og_redeem_r1cs / owshen_amd/circuit.py redeem_r1cs (the R1CS):
 *   n_wires = 1887 + 3 depth + (6 + depth) 730, n_constraints = 2019 + 2 depth + (6 + depth) 730 (29 723 / 29 823 at depth 32:
 *   domain 2^15).  depth 1..64; n <= 65 535 per og_redeem_witness_d call.  shape[0..2] = n_wires, n_constraints, n_pub.
 * inputs_d: n records of (8 + depth) x 32 B canonical little-endian:
 *   x | amount | recipient | amount_out | token | chain_id | change_commitment | index (u64, low bytes) | siblings[depth]
 * witness_out_d: n x n_wires x 32 B.  og_redeem_prove_batch_d: records -> proofs (rs: n x 64 B host, proofs_out: n x 256 B host,
 * public_out (host, may be NULL): n x 7 x 32 B in verifier order).  Same bytes as og_redeem_witness_d + og_prove_batch_d.  The key must
 * have this shape's wire count and n_pub (a split key has the n_pub and is refused by its wire count).
 * OG_ERR_INVALID, before anything is proved: a malformed record; og_last_error names the record and its lowest offending field
 * ("input record 3: field 3 (amount_out)"; 0 x, 1 amount, 2 recipient, 3 amount_out, 4 token, 5 chain_id, 6 change_commitment,
 * 7 index, 8 + l sibling l): any field >= r; field 0 if x >= l; field 1 if amount >= 2^128; field 3 if amount_out >= 2^128 or
 * amount_out > amount (compared as integers); field 7 if the index does not fit the tree.
 * One walk, one lane per request whatever n, as the send statement.  Out of scope: a wave-wide walk, host chains, a submit / job
 * form, a multi-GPU and a window-sharded form, and Rust and Solidity bindings (ffi/ and contracts/ are frozen). */
int og_redeem_shape(int depth, uint64_t shape[3]);
int og_redeem_witness_d(og_ctx* ctx, int depth, const uint8_t* inputs_d, size_t n, uint8_t* witness_out_d);
int og_redeem_prove_batch_d(og_ctx* ctx, const og_pk* pk, int depth, const uint8_t* inputs_d, size_t n, const uint8_t* rs,
                            uint8_t* proofs_out, uint8_t* public_out);

/* The same call in two halves, for a host that keeps requests flowing (a sequencer proving batch after batch): submit
 * enqueues ALL the work of the batch on the ctx's streams and returns; og_job_wait blocks until it is done, fills
 * proofs_out / public_out (which, like rs, must stay valid until then) and frees the job.  At most two calls may be in
 * flight on a ctx, and they complete in submission order.  Submitting batch k + 1 before waiting for batch k lets its cold
 * start (first witnesses, sparse products, sorts) run beside batch k's last bucket accumulations instead of after them
 * (measured: +0.7 % proofs/s at batch 1024 -- the chip is already busy, what is gained is the latency of the first
 * witnesses and of the copy-out).  og_job_wait returns what og_withdraw_prove_batch_d would have (OG_ERR_UNSATISFIED ...).
 * The overlap exists for batches the library runs through its stage pipeline (sub-batches of >= 64 proofs: og_prove_plan mode
 * 3).  A smaller call (modes 1 / 2: what a request coalescer produces under light load) shares scratch with its predecessor
 * without per-slot guards, so its submit first waits -- holding the ctx -- until the call before it has finished: submit k + 1
 * then returns when batch k is done, and og_job_poll / other ctx calls from other threads queue behind it meanwhile.  Nothing
 * is lost against blocking calls (such batches take milliseconds); the call-ahead gain is a property of large batches.
 * Submit itself never proves: also a call that fits one sub-batch enqueues its witnesses with the rest and returns (until the
 * end of round 6 a small statement's witnesses were generated before the enqueue, with the host waiting for them).
 * While a thread is inside og_job_wait for a job, og_job_abandon and a second og_job_wait on that job are refused, and
 * og_shutdown waits for the waiter; og_msm_d / og_msm_windows_d / og_msm_combine_d, og_pk_load_rows and og_pk_load of a key that
 * takes the evaluation form are refused while a submitted call is pending (they use the same scratch). */
typedef struct og_job og_job;
int og_withdraw_prove_batch_submit_d(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2,
                                     const uint8_t* inputs_d, size_t n, const uint8_t* rs, uint8_t* proofs_out,
                                     uint8_t* public_out, og_job** job_out);
int og_job_wait(og_ctx* ctx, og_job* job);
/* Non-blocking: *done_out = 1 once every kernel of the job has finished (og_job_wait would then return at once), else 0.  The
 * job stays pending either way.  Threading: og_job_wait blocks WITHOUT holding the context's lock, so one host thread may sit
 * in og_job_wait for batch k while another submits batch k + 1 -- the shape of a request coalescer that keeps one call ahead
 * from a blocking-task pool; a single-threaded host polls instead. */
int og_job_poll(og_ctx* ctx, og_job* job, int* done_out);
/* Every job must be consumed exactly once: by og_job_wait, or -- when the caller no longer wants the results, e.g. its
 * output buffers are going away -- by og_job_abandon, which waits for the job's kernels (they write device scratch the next
 * call reuses), copies nothing out and frees the call slot.  A handle that is not a pending job of this ctx (already
 * consumed, another ctx's) is refused with OG_ERR_INVALID by both. */
int og_job_abandon(og_ctx* ctx, og_job* job);

/* Window-sharded proving for a host that runs ONE PROCESS PER GPU and owns the collective (torch.distributed over RCCL:
 * owshen_amd/shard.py; og_multi_*_prove_sharded above is the same composition inside one process):
 *   og_withdraw_prove_partials_d / og_prove_partials_d   the front half on this rank: witnesses (or the caller's, device),
 *       sparse products, quotient, and the windows k = win_rank (mod win_world) of the five queries.  partials_d (device,
 *       n x OG_PARTIAL_BYTES): five arrays, A | B1 | L | H (n x 128 B: extended-Jacobian XYZZ over Fq, Montgomery form, the
 *       library's internal point format -- opaque to the host, only moved) | B2 (n x 256 B).  Blocking; errors and public_out
 *       as og_withdraw_prove_batch_d (every rank sees the same inputs, so every rank reports the same error).
 *   -- the host all-gathers the ranks' blocks: gathered_d = win_world x n x OG_PARTIAL_BYTES, rank-major --
 *   og_prove_from_partials_d   adds the ranks' shares query by query, applies the blinding rs (n x 64 B host) and writes the
 *       n x 256 B proofs (host): byte-identical to og_withdraw_prove_batch_d / og_prove_batch_d on the same inputs.  Any
 *       rank may run it (all hold the gathered block); the others skip it. */
#define OG_PARTIAL_BYTES 768
int og_withdraw_prove_partials_d(og_ctx* ctx, const og_pk* pk, int depth, uint64_t n_pad3, uint64_t n_pad2,
                                 const uint8_t* inputs_d, size_t n, int win_rank, int win_world, uint8_t* partials_d,
                                 uint8_t* public_out);
int og_prove_partials_d(og_ctx* ctx, const og_pk* pk, const uint8_t* witnesses_d, size_t n, int win_rank, int win_world,
                        uint8_t* partials_d);
int og_prove_from_partials_d(og_ctx* ctx, const og_pk* pk, const uint8_t* gathered_d, int win_world, size_t n,
                             const uint8_t* rs, uint8_t* proofs_out);

/* ---- key material: the withdraw circuit and Groth16 key generation (what a Rust host needs to obtain an OWPK0001 /
 * OWVK0001 blob without any Python) ----------------------------------------------------------------------------
 * og_r1cs: host-side R1CS, constraint rows only (the library appends the n_pub + 1 input-consistency rows), CSR per matrix
 * (A = 0, B = 1, C = 2) with canonical 32-byte coefficients.
 *   og_withdraw_r1cs  the statement of og_withdraw_witness_d: depth-`depth` MiMC7 Merkle withdraw circuit + n_pad3 / n_pad2
 *                     synthetic gates; dense != 0 appends the two density rows (every wire gets an A and a B base).
 *                     Wire and row order are specified by oracle/py/withdraw.py.
 *   og_r1cs_from_csr  any other circuit: ptr[k] has n_constraints + 1 entries.
 *   og_r1cs_info      info[0..5] = n_wires, n_pub, n_constraints, nnz_a, nnz_b, nnz_c
 *   og_r1cs_export    copies matrix k out (buffers sized from og_r1cs_info)
 *   og_setup          Groth16 key generation from explicit toxic waste tau | alpha | beta | gamma | delta (5 x 32 B, canonical,
 *                     non-zero; tests and benchmarks -- a production key comes from a ceremony), computed on the GPU.
 *                     *pk_out / *vk_out are malloc'd blobs in the OWPK0001 / OWVK0001 formats; release with og_blob_free. */
typedef struct og_r1cs og_r1cs;
int og_withdraw_r1cs(og_ctx* ctx, int depth, uint64_t n_pad3, uint64_t n_pad2, int dense, og_r1cs** out);
/* the statement of og_deposit_witness_d (wire and row order: oracle/py/deposit.py) */
int og_deposit_r1cs(og_ctx* ctx, og_r1cs** out);
/* the statement of og_split_witness_d at this depth (wire and row order: tests/split_spec.py) */
int og_split_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
/* the statement of og_join_witness_d at this depth (wire and row order: tests/join_spec.py) */
int og_join_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
/* the statement of og_transfer_witness_d at this depth (wire and row order: tests/transfer_spec.py) */
int og_transfer_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
/* the statement of og_claim_witness_d at this depth (wire and row order: tests/claim_spec.py) */
int og_claim_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
/* the statement of og_send_witness_d at this depth (wire and row order: tests/send_spec.py) */
int og_send_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
/* the statement of og_redeem_witness_d at this depth (wire and row order: tests/redeem_spec.py) */
int og_redeem_r1cs(og_ctx* ctx, int depth, og_r1cs** out);
int og_r1cs_from_csr(uint64_t n_wires, uint64_t n_pub, uint64_t n_constraints, const uint32_t* const ptr[3],
                     const uint32_t* const col[3], const uint8_t* const val[3], og_r1cs** out);
void og_r1cs_free(og_r1cs* r1cs);
int og_r1cs_info(const og_r1cs* r1cs, uint64_t info[6]);
int og_r1cs_export(const og_r1cs* r1cs, int matrix, uint32_t* ptr_out, uint32_t* col_out, uint8_t* val_out);
int og_setup(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t toxic[160], uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out,
             size_t* vk_len);
/* og_setup plus the OWPR0001 row-basis extension of the key (see og_pk_load_rows) */
int og_setup_rows(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t toxic[160], uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out,
                  size_t* vk_len, uint8_t** rows_out, size_t* rows_len);
void og_blob_free(uint8_t* blob);

/* ---- snarkjs' files at the boundary (owshen_amd/csrc/zkey.hip; oracle/py/zkey.py restates the formats and is the oracle) ----
 * The lineage BASELINE.json's north_star names proved with circom / snarkjs; its keys are `.zkey` files, its witnesses `.wtns`
 * files (iden3 binfile containers).  No reference interface to replace: the snapshot holds no key; the
 * caller would be the node's start-up beside /root/reference/src/cli/node.rs:26-53.
 *   og_zkey_import  a Groth16 BN254 .zkey -> malloc'd "OWPK0001" / "OWVK0001" blobs (og_blob_free) for og_pk_load / og_verify.
 *                   Points leave the file's Montgomery form, the rows move from ffjavascript's root order to this library's, the
 *                   odd-coset Lagrange H section becomes the coefficient-basis H query through a DFT over G1 points on the
 *                   GPU, and the key carries header flag 1: a .zkey has no C matrix, the prover takes C z = (A z) o (B z) as
 *                   snarkjs does -- so a witness that violates a constraint is NOT refused (OG_ERR_UNSATISFIED needs a C
 *                   matrix), its proof simply does not verify.  Refused with OG_ERR_INVALID: another curve or protocol, a
 *                   section whose length disagrees with the header, a coordinate >= q, a point off its curve, a coefficient
 *                   >= r or outside the matrix.  Proofs made with the imported key are the ones snarkjs' prover makes for
 *                   the same (r, s).  Subgroup membership of the key's G2 points is not checked here (it would change what
 *                   this call refuses): a key that passes og_pk_verify, below, has all of them in the order-r subgroup.
 *                   r1cs (optional, may be NULL): the circuit the key was made for, as og_r1cs_read returns it.  Its A and B must
 *                   be the key's coefficient section row for row (else OG_ERR_INVALID: not this key's circuit); its C matrix
 *                   then rides in the imported key (flag 0) and OG_ERR_UNSATISFIED works as for a key of og_setup.
 *   og_r1cs_read    circom's .r1cs (iden3 r1csfile, version 1) -> og_r1cs (og_r1cs_free); n_pub = nPubOut + nPubIn; host only.
 *   og_r1cs_write   the inverse (malloc'd, og_blob_free): what `snarkjs r1cs info` / `snarkjs groth16 setup` read.
 *   og_zkey_export  the way back: an OWPK0001 + OWVK0001 pair as a .zkey that `snarkjs groth16 prove` accepts (C matrix left
 *                   behind, H section by the inverse transform, "no contributions": `snarkjs zkey verify` against a .ptau
 *                   will not pass, proving and verifying do, and so does og_pk_verify after an import beside the .r1cs).
 *   og_wtns_read    a .wtns -> n x 32 B canonical values (values_out == NULL: only *n_out); host only, no og_ctx.
 *   og_wtns_write   the inverse (malloc'd, og_blob_free).
 * The formats are written down from the published sources of snarkjs 0.7 / ffjavascript; no file made by snarkjs itself was
 * available to test against. */
int og_zkey_import(og_ctx* ctx, const uint8_t* zkey, size_t zkey_len, const og_r1cs* r1cs, uint8_t** pk_out, size_t* pk_len,
                   uint8_t** vk_out, size_t* vk_len);
int og_zkey_export(og_ctx* ctx, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, uint8_t** zkey_out,
                   size_t* zkey_len);
int og_r1cs_read(const uint8_t* r1cs_file, size_t len, og_r1cs** out);
int og_r1cs_write(const og_r1cs* r1cs, uint8_t** file_out, size_t* file_len);
int og_wtns_read(const uint8_t* wtns, size_t len, uint8_t* values_out, size_t capacity, uint64_t* n_out);
int og_wtns_write(const uint8_t* values, uint64_t n, uint8_t** wtns_out, size_t* wtns_len);

/* ---- a key from a ceremony: `snarkjs groth16 setup` on the GPU, and the delta step (owshen_amd/csrc/ptau.hip) ----------------
 * og_setup takes the toxic waste as plain scalars; these calls never see a secret scalar.  With og_zkey_export the file loop
 * closes: .r1cs + .ptau -> OWPK0001 / OWVK0001 -> .zkey.  No reference interface to replace.
 *   og_ptau_info      host only, no og_ctx: info[0..3] = power, ceremony power, tauG1 points present (section 2's bytes / 64), 1 if
 *                     the prepared Lagrange sections 12..15 are all present (they are never read).
 *   og_setup_ptau     an R1CS + a BN254 .ptau -> malloc'd OWPK0001 / OWVK0001 blobs (og_blob_free) with gamma = delta = 1 --
 *                     snarkjs' initial zkey; byte for byte og_setup(r1cs, tau, alpha, beta, 1, 1) for the file's (tau, alpha,
 *                     beta).  The file: iden3 binfile "ptau", version <= 1; section 1 = u32 n8 (32) | q | u32 power | u32
 *                     ceremonyPower; 2 = tauG1, 2^(power+1) - 1 points; 3 = tauG2, 2^power; 4 = alphaTauG1; 5 = betaTauG1; 6 =
 *                     betaG2 (one point); any other section (7: contributions, 12..15: Lagrange forms) is skipped.  Points are
 *                     uncompressed affine, little-endian Montgomery numbers with R = 2^256, G2 as x.c0 | x.c1 | y.c0 | y.c1, all
 *                     zeros = infinity (the .zkey encoding).  With d = 2^log_d the key's domain (constraints + n_pub + 1 rows),
 *                     the call needs power >= log_d and reads the first d entries of sections 3..5 and 2 d - 1 of section 2.
 *                     On the GPU: four inverse DFTs of size d over POINTS (three in G1, one in G2: the Lagrange bases at this
 *                     library's root 7^((r-1)/d)), the transposed sparse products of A, B, C with those bases (a lane per
 *                     non-zero, then a segmented sum), one subtraction per H entry.  Header flag 0: the C matrix rides in the key.
 *                     Refused with OG_ERR_INVALID, the reason naming the section: another base field, a missing or mis-sized
 *                     section, power < log_d, a coordinate >= q, a point off its curve, tauG1[0] / tauG2[0] not the generators,
 *                     a used G2 point (tauG2, betaG2) outside the order-r subgroup.  NOT checked: that the file is a valid
 *                     ceremony (the pairing checks between consecutive powers) -- that is og_ptau_verify's job, below.
 *   og_pk_contribute  the delta step of phase 2: delta <- delta * d, L and H queries <- (1 / d) *; everything else is copied (the
 *                     header flag too).  d: 32 B canonical, non-zero, < r.  Any OWPK0001 / OWVK0001 pair: og_setup's,
 *                     og_setup_ptau's, an imported one.  After og_setup_ptau the result is og_setup(.., gamma = 1, delta = d) byte
 *                     for byte.  The library draws no randomness: d is the caller's, and so is forgetting it.  No contribution
 *                     transcript is written (snarkjs' challenge hashes are out of scope): og_zkey_export still says "no
 *                     contributions".
 *   og_ptau_verify    `snarkjs powersoftau verify` without the contribution transcripts (section 7 is not read): is every
 *                     section a geometric sequence in the ratio tauG2[1] carries?  OG_OK means the verdict is in *failed_out: 0 if
 *                     everything holds, otherwise one bit per failed check -- every check runs, the mask is complete, and
 *                     og_last_error() names the failed checks.  With rho_i the challenge scalars below, N the points of a section,
 *                     S0 = sum_{i<N-1} rho_i P_i and S1 = sum_{i<N-1} rho_i P_{i+1}:
 *                        1  tauG1:       e(S1, G2) = e(S0, tauG2[1])         4  alphaTauG1: the same
 *                        2  tauG2:       e(tauG1[1], S0) = e(G1, S1)         8  betaTauG1:  the same
 *                       16  betaG2:      e(betaTauG1[0], G2) = e(G1, betaG2)
 *                     A point at infinity anywhere in a section sets that section's bit (no ceremony holds one).  Malformed
 *                     input is OG_ERR_INVALID with og_setup_ptau's reasons, here for EVERY point of sections 2..6, not a prefix.
 *                     On the GPU: per section one vector of scalars, one digit sort, two sums over plain bases (from point 0,
 *                     from point 1); on the host: one two-pairing product per check.
 *   og_pk_verify      `snarkjs zkey verify`, likewise: is (pk, vk) the key of THIS circuit from THIS file, up to its delta?  The
 *                     delta = 1 key (pk0, vk0) is rebuilt as og_setup_ptau builds it (same refusals), then, as bits of *failed_out:
 *                        1  header, domain, matrices, alpha1, beta1, beta2 of pk equal pk0's; alpha, beta, gamma of vk equal
 *                           vk0's; lengths equal     2  the A, B1, B2 queries are pk0's, byte for byte     4  vk's IC is vk0's
 *                        8  delta1, delta2 not infinity, canonical, on their curves, delta2 in the order-r subgroup, pk's delta2 =
 *                           vk's, e(delta1, G2) = e(G1, delta2)
 *                       16  L: every entry canonical and on the curve, e(sum rho_i L_i, delta2) = e(sum rho_i L0_i, G2)
 *                       32  H: the same over the H query
 *                     If delta2 itself is unusable (infinity, off the twist, outside the subgroup) 16 and 32 are set with 8; if the
 *                     header or a length differs from pk0's no query lies where it should and every bit is set.  A key with
 *                     header flag 1 (imported without its .r1cs) is OG_ERR_INVALID: import it beside its .r1cs.  A key that
 *                     passes has every G2 element in the subgroup (bits 1, 2 and 8 cover them).  Accepts og_setup_ptau's key,
 *                     any number of og_pk_contribute steps on it, og_setup(.., gamma = 1, any delta) for the file's (tau, alpha,
 *                     beta), and such a key after og_zkey_export / og_zkey_import with its r1cs.
 *                     Both calls are refused while a submitted prove call is pending (they use the lone MSM's scratch).
 *                     The challenge scalars: the library draws no randomness, so they are Fiat-Shamir.  seed = keccak256(tag |
 *                     keccak256(ptau) [| keccak256(pk) | keccak256(vk)]) mod r -- every byte of the inputs, so whoever wrote them
 *                     could not know the scalars --, rho_i = the low 128 bits of MiMC7 hash2(seed, section * 2^32 + i), computed
 *                     on the device.  A section that is NOT what it should be passes only if its points satisfy one linear
 *                     relation in the rho_i: probability about 2^-128.
 * The .ptau format is written down from the published sources of snarkjs 0.7; no file made by snarkjs itself was available to
 * test against: the tests build their files from a known (tau, alpha, beta). */
int og_ptau_info(const uint8_t* ptau, size_t len, uint64_t info[4]);
int og_setup_ptau(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t* ptau, size_t len, uint8_t** pk_out, size_t* pk_len,
                  uint8_t** vk_out, size_t* vk_len);
int og_pk_contribute(og_ctx* ctx, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t d[32],
                     uint8_t** pk_out, size_t* pk_out_len, uint8_t** vk_out, size_t* vk_out_len);
int og_ptau_verify(og_ctx* ctx, const uint8_t* ptau, size_t len, uint32_t* failed_out);
int og_pk_verify(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t* ptau, size_t len, const uint8_t* pk, size_t pk_len,
                 const uint8_t* vk, size_t vk_len, uint32_t* failed_out);

/* ---- key-generation helpers (trusted setup from explicit toxic waste; tests and bench) --------
 * out[i] = k_i * base.  base: host, canonical affine; scalars_d / out_d: device, canonical. */
int og_scalar_mul_d(og_ctx* ctx, int group, const uint8_t* base, const uint8_t* scalars_d, size_t n,
                    uint8_t* out_d);
/* Lagrange basis of the size-2^log_d NTT domain evaluated at tau: out[k] = L_k(tau), d x 32 B canonical, in the natural order of
 * the domain (L_k belongs to w^k).  A tau inside the domain, tau = w^j, gives the unit vector: out[j] = 1, every other element 0.
 * tau: host, canonical; a tau >= r is refused with OG_ERR_INVALID, it is never reduced mod r. */
int og_lagrange_evals_d(og_ctx* ctx, int log_d, const uint8_t tau[32], uint8_t* out_d);
/* out[row] = sum_k val[k] * x[col[k]] over Fr, CSR with canonical values */
int og_spmv_fr_d(og_ctx* ctx, const uint32_t* row_ptr_d, const uint32_t* col_d, const uint8_t* val_d,
                 size_t n_rows, const uint8_t* x_d, uint8_t* out_d);

/* ---- region timing (HIP events on the ctx stream; for bench.py's roofline figures) ------------
 * og_profile(ctx, 1) clears the log and starts recording; og_profile(ctx, 0) stops.
 * og_profile_read: out[0] = total milliseconds, out[1] = number of regions, out[2] = units processed.
 * kind: 0 bucket accumulation G1 (one kernel launch per region; units = points x proofs), 1 same for G2,
 *       2 H-polynomial pipeline (units = domain elements), 3 digit sort (scalars), 4 / 5 bucket reduction
 *       G1 / G2 (buckets), 6 witness generation (witnesses), 7 R1CS sparse products (non-zeros),
 *       8 proof assembly (proofs), 9 / 10 heavy-bucket accumulation G1 / G2 (buckets above 2048 entries: a workgroup per
 *       bucket segment; a lone 2^26-point MSM is accumulated entirely here; units = points x proofs). */
int og_profile(og_ctx* ctx, int enable);
/* The batched prover pipelines its sub-batches over two HIP streams (memory-bound preparation of sub-batch k + 1 under
 * the VALU-bound arithmetic of k; scratch per sub-batch parity; default 2).  1 = strictly serial on one stream: kernel
 * timings free of co-scheduling. */
int og_set_lanes(og_ctx* ctx, int n_lanes);
int og_profile_read(og_ctx* ctx, int kind, double out[3]);
/* Frees the ctx's scratch arena (it regrows on demand): a long-lived host that proved a large batch hands the tens of GB of
 * sub-batch scratch back before, say, building 2^26-point window tables.  Waits for the ctx's streams first. */
int og_release_scratch(og_ctx* ctx);
/* Bound the HBM the prover reserves for sub-batch scratch on this ctx: the stage pipeline rotates over two scratch slots, each
 * sized for one sub-batch (~230 MB per proof of the 2^18-wire circuit, at most 256 proofs: ~70 GB at batch 1024 by default, or
 * 0.85 x the free memory if that is less); with a budget the sub-batches shrink until two slots fit into `bytes` (never below
 * one proof per sub-batch).  0 restores the default.  Takes effect from the next call; scratch already reserved stays until
 * og_release_scratch.  The environment variable OG_SUB_BATCH (a cap in proofs) remains as the operator's coarse knob. */
int og_set_scratch_budget(og_ctx* ctx, uint64_t bytes);
/* Latency knob for a host that proves a HANDFUL of requests per call (the reference's handler proves one per HTTP call,
 * /root/reference/src/services/api_services/withdraw.rs:27-71): withdraw calls of at most `max_requests` requests (0 .. 64;
 * default 0 = never) walk their MiMC7 chains on the HOST CPU -- one thread per request, the library's own field layer compiled
 * for the host, the wires copied up -- instead of on a lone GPU wave.  A request's walk is ~19 000 dependent modular products; a
 * lone wave takes ~0.42 us for each, a server core 20-50 ns: one request 10.7 -> ~4.5 ms.  Everything else of the call (padding
 * gates, sparse products, quotient, MSMs, assembly) stays on the GPU, larger calls are untouched, the bytes are the same.
 * og_mimc7_append_d follows the same bound for its leaves: an append of at most `max_requests` leaves hashes on the host (one
 * leaf into a depth-32 tree: 8.6 -> 0.32 ms).
 * Not a fallback: the call still fails without a GPU. */
int og_set_host_chains(og_ctx* ctx, int max_requests);
/* HBM accounting: out[0] = bytes of scratch this ctx's arena currently holds (sub-batch slots, call-level buffers, NTT
 * tables), out[1] = number of arena buffers, out[2] / out[3] = free / total bytes of the device (hipMemGetInfo). */
int og_mem_info(og_ctx* ctx, uint64_t out[4]);
/* How a call of n proofs with this key is scheduled on this ctx right now (it depends on the free HBM): sizes_out[0 .. *count_out)
 * = the sub-batches (at most `cap` are written), *mode_out = 0 one stream, serial; 1 a call of <= 16 requests, its five queries fanned out over the streams;
 * 2 whole sub-batches side by side on two streams; 3 the stage pipeline. */
int og_prove_plan(og_ctx* ctx, const og_pk* pk, size_t n, uint32_t* sizes_out, size_t cap, size_t* count_out, int* mode_out);
/* The GLV decomposition the library uses for the proof assembly of latency-bound calls, as a host function (no ctx, no GPU):
 * k (32 B LE, canonical) = k1 + lambda k2 (mod r) with |k1|, |k2| < 2^127, lambda the eigenvalue of the BN254 G1
 * endomorphism (x, y) -> (beta x, y).  out = |k1| (16 B LE, bit 127 = sign) || |k2| (the same).  Exposed so that the
 * constants can be checked from outside (tests/test_glv.py re-derives lambda from the modulus). */
int og_glv_decompose(const uint8_t k[32], uint8_t out[32]);
/* bytes of HBM a loaded proving key occupies (CSR matrices + the five per-window query tables + wire maps) */
int og_pk_bytes(const og_pk* pk, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* OWSHEN_GPU_H */
