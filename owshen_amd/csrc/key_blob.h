// The OWPK0001 (proving key) and OWVK0001 (verifying key) blobs in code: the one reader and the one writer of the two formats
// include/owshen_gpu.h specifies.  Host code only, no HIP call: verify.hip includes it and still links with g++ alone.  Every
// translation unit gets its own copy (anonymous namespace, as verify_tower.h).
//
// Proving key, all little-endian, every section after the header padded to a multiple of 32 B on its own:
//   u64 x 10 : magic, n_wires, n_pub, log_d, n_rows, nnz_a, nnz_b, nnz_c, flags, 0
//              flags bit 0: the key carries no C matrix (nnz_c = 0) and the prover takes C z = (A z) o (B z) row by row -- what
//              snarkjs' prover does, whose .zkey stores A and B only (og_zkey_import); such a key cannot tell a witness that
//              violates a constraint (the proof simply does not verify), only wire 0 != 1
//   alpha_g1 (64) beta_g1 (64) delta_g1 (64) pad (64) | beta_g2 (128) delta_g2 (128)
//   for M in A, B, C: ptr (n_rows+1 u32) | col (nnz u32) | val (nnz x 32 B canonical)
//   a_query (m x 64) | b_g1_query (m x 64) | b_g2_query (m x 128) | l_query ((m-n_pub-1) x 64) | h_query ((d-1) x 64)
// Verifying key: magic | u64 n_pub | alpha_g1 (64) | beta_g2 (128) | gamma_g2 (128) | delta_g2 (128) | IC ((n_pub+1) x 64)
//
// pk_view / vk_view make the structural checks every consumer shares; what only one consumer asks (the header flags, the CSR,
// the domain bound of a .zkey) stays at that consumer's call site.
#pragma once
#include "ctx.h"
#include <string.h>
#include <string>
#include <vector>

namespace og {

struct QapRows {  // constraints, then the n_pub + 1 input-consistency rows; CSR, canonical values
  std::vector<uint32_t> ptr[3], col[3];
  std::vector<uint8_t> val[3];
};

struct KeyParts {  // canonical affine bytes on the host
  size_t m = 0, l = 0, n_rows = 0;
  int log_d = 0;
  uint64_t flags = 0;  // header word 8
  const uint8_t *alpha1 = nullptr, *beta1 = nullptr, *delta1 = nullptr, *beta2 = nullptr, *gamma2 = nullptr, *delta2 = nullptr;
  const uint8_t* query[5] = {};  // A (m) | B in G1 (m) | B in G2 (m) | L (m - l - 1) | H (2^log_d - 1)
  const uint8_t* ic = nullptr;   // l + 1
};

namespace {

constexpr uint64_t PK_MAGIC = 0x313030304b50574full;  // "OWPK0001"
constexpr char VK_MAGIC[9] = "OWVK0001";
// proving key: the header, then two blocks of 256 B with the constants
constexpr size_t PK_HEADER = 80, PK_FIXED = 80 + 512;
constexpr size_t PK_CONSTS1 = PK_HEADER, PK_CONSTS2 = PK_HEADER + 256;
constexpr size_t PK_ALPHA1 = PK_CONSTS1, PK_BETA1 = PK_CONSTS1 + 64, PK_DELTA1 = PK_CONSTS1 + 128;
constexpr size_t PK_BETA2 = PK_CONSTS2, PK_DELTA2 = PK_CONSTS2 + 128;
constexpr size_t PK_FLAGS = 64, PK_WORD9 = 72;  // header words 8 and 9
// verifying key: magic, n_pub, alpha1, then beta2 | gamma2 | delta2; IC follows the fixed part
constexpr size_t VK_FIXED = 16 + 64 + 3 * 128;
constexpr size_t VK_ALPHA1 = 16, VK_BETA2 = VK_ALPHA1 + 64, VK_GAMMA2 = VK_BETA2 + 128, VK_DELTA2 = VK_GAMMA2 + 128, VK_IC = VK_FIXED;

inline size_t pad32(size_t n) { return (n + 31) / 32 * 32; }
inline void put_padded(std::vector<uint8_t>& out, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  out.insert(out.end(), b, b + n);
  out.resize(out.size() + (pad32(n) - n), 0);  // every section is padded to a multiple of 32 B on its own
}
// a caller's blob has no alignment: every word is read through memcpy
inline uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}
inline uint64_t rd64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
inline bool all_zero(const uint8_t* p, size_t n) {  // (a point: the point at infinity)
  for (size_t i = 0; i < n; i++)
    if (p[i]) return false;
  return true;
}

// ---- the reader ---------------------------------------------------------------------------------------------------------------
struct PkView {
  const uint8_t* blob;
  size_t len;
  uint64_t m, l, log_d, n_rows, nnz[3], flags, word9;  // the header after its magic
  size_t d, nl, nh;                                     // 2^log_d, m - l - 1, d - 1
  const uint8_t *alpha1, *beta1, *delta1, *beta2, *delta2;
  const uint8_t *ptr[3], *col[3], *val[3];  // A, B, C
  const uint8_t* query[5];                  // A | B in G1 | B in G2 | L | H
  size_t q_n[5], q_bytes[5];                // points and bytes of each, without the padding
  size_t off(const uint8_t* p) const { return (size_t)(p - blob); }
};

inline bool pk_is_blob(const uint8_t* blob, size_t len) { return len >= PK_FIXED && rd64(blob) == PK_MAGIC; }
inline bool vk_is_blob(const uint8_t* vk, size_t len) { return len >= VK_FIXED && memcmp(vk, VK_MAGIC, 8) == 0; }

// The structure of a proving key: header in range, every section inside the blob, the length the header implies.  Says nothing
// about header words 8 and 9, about what the CSR sections hold or about the points.
inline int pk_view(const uint8_t* blob, size_t len, const std::string& who, PkView* v) {
  OG_REQUIRE(pk_is_blob(blob, len), who + ": not an OWPK0001 blob");
  v->blob = blob;
  v->len = len;
  v->m = rd64(blob + 8); v->l = rd64(blob + 16); v->log_d = rd64(blob + 24); v->n_rows = rd64(blob + 32);
  for (int k = 0; k < 3; k++) v->nnz[k] = rd64(blob + 40 + 8 * k);
  v->flags = rd64(blob + PK_FLAGS);
  v->word9 = rd64(blob + PK_WORD9);
  OG_REQUIRE(v->log_d >= 1 && v->log_d <= 28, who + ": log_d must be 1..28");
  OG_REQUIRE(v->m >= 1 && v->m < (1ull << 31) && v->l < v->m, who + ": bad wire counts");
  v->d = (size_t)1 << v->log_d;
  v->nl = v->m - v->l - 1;
  v->nh = v->d - 1;
  OG_REQUIRE(v->n_rows <= v->d, who + ": more QAP rows than the domain holds");
  v->alpha1 = blob + PK_ALPHA1; v->beta1 = blob + PK_BETA1; v->delta1 = blob + PK_DELTA1;
  v->beta2 = blob + PK_BETA2; v->delta2 = blob + PK_DELTA2;
  size_t off = PK_FIXED;
  for (int k = 0; k < 3; k++) {
    OG_REQUIRE(v->nnz[k] < (1ull << 32), who + ": nnz too large");
    v->ptr[k] = blob + off; off += pad32((v->n_rows + 1) * 4);
    v->col[k] = blob + off; off += pad32(v->nnz[k] * 4);
    v->val[k] = blob + off; off += pad32(v->nnz[k] * 32);
    OG_REQUIRE(off <= len, who + ": truncated R1CS section");
  }
  const size_t q_n[5] = {(size_t)v->m, (size_t)v->m, (size_t)v->m, v->nl, v->nh};
  const size_t q_pb[5] = {64, 64, 128, 64, 64};
  for (int k = 0; k < 5; k++) {
    v->query[k] = blob + off;
    v->q_n[k] = q_n[k];
    v->q_bytes[k] = q_n[k] * q_pb[k];
    off += pad32(v->q_bytes[k]);
  }
  OG_REQUIRE(off == len, who + ": blob length does not match its header");
  return OG_OK;
}

// the first n_matrices of A, B, C are well-formed CSR over m columns: nothing built from them can index out of bounds
inline int pk_csr_check(const PkView& v, int n_matrices, const std::string& who) {
  for (int k = 0; k < n_matrices; k++) {
    const uint8_t *p = v.ptr[k], *c = v.col[k];
    OG_REQUIRE(rd32(p) == 0 && rd32(p + v.n_rows * 4) == v.nnz[k], who + ": CSR row pointers inconsistent");
    for (size_t r = 0; r < v.n_rows; r++) OG_REQUIRE(rd32(p + r * 4) <= rd32(p + r * 4 + 4), who + ": CSR row pointers not monotone");
    for (size_t i = 0; i < v.nnz[k]; i++) OG_REQUIRE(rd32(c + i * 4) < v.m, who + ": CSR column out of range");
  }
  return OG_OK;
}

struct VkView {
  uint64_t n_pub;
  const uint8_t *alpha1, *beta2, *gamma2, *delta2, *ic;  // ic: n_pub + 1 points
};

inline int vk_view(const uint8_t* vk, size_t len, const std::string& who, VkView* v) {
  OG_REQUIRE(vk_is_blob(vk, len), who + ": bad verifying key (want OWVK0001)");
  v->n_pub = rd64(vk + 8);
  OG_REQUIRE(v->n_pub <= ((uint64_t)1 << 24), who + ": too many public inputs");  // also keeps (n_pub + 1) * 64 from wrapping
  OG_REQUIRE(len == VK_FIXED + (v->n_pub + 1) * 64, who + ": verifying key length does not match its header");
  v->alpha1 = vk + VK_ALPHA1; v->beta2 = vk + VK_BETA2; v->gamma2 = vk + VK_GAMMA2; v->delta2 = vk + VK_DELTA2; v->ic = vk + VK_IC;
  return OG_OK;
}

// the verifying key counts the proving key's public inputs and carries its alpha, beta and delta
inline bool vk_is_of_pk(const VkView& vk, const PkView& pk) {
  return vk.n_pub == pk.l && memcmp(vk.alpha1, pk.alpha1, 64) == 0 && memcmp(vk.beta2, pk.beta2, 128) == 0 && memcmp(vk.delta2, pk.delta2, 128) == 0;
}

// ---- the writer ---------------------------------------------------------------------------------------------------------------
// both blobs from canonical group elements; rows: n_rows + 1 pointers per matrix
inline void key_blobs(const KeyParts& k, const QapRows& rows, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk) {
  pk.clear();
  const uint64_t head[10] = {PK_MAGIC, k.m, k.l, (uint64_t)k.log_d, k.n_rows, rows.col[0].size(), rows.col[1].size(), rows.col[2].size(), k.flags, 0};
  pk.insert(pk.end(), (const uint8_t*)head, (const uint8_t*)head + PK_HEADER);  // the header is not padded
  put_padded(pk, k.alpha1, 64);
  put_padded(pk, k.beta1, 64);
  put_padded(pk, k.delta1, 64);
  pk.resize(pk.size() + 64, 0);
  put_padded(pk, k.beta2, 128);
  put_padded(pk, k.delta2, 128);
  for (int q = 0; q < 3; q++) {
    put_padded(pk, rows.ptr[q].data(), rows.ptr[q].size() * 4);
    put_padded(pk, rows.col[q].data(), rows.col[q].size() * 4);
    put_padded(pk, rows.val[q].data(), rows.val[q].size());
  }
  const size_t nl = k.m - k.l - 1, nh = ((size_t)1 << k.log_d) - 1;
  const size_t q_bytes[5] = {k.m * 64, k.m * 64, k.m * 128, nl * 64, nh * 64};
  for (int q = 0; q < 5; q++) put_padded(pk, k.query[q], q_bytes[q]);
  vk.clear();
  vk.insert(vk.end(), (const uint8_t*)VK_MAGIC, (const uint8_t*)VK_MAGIC + 8);
  const uint64_t npub = k.l;
  vk.insert(vk.end(), (const uint8_t*)&npub, (const uint8_t*)&npub + 8);
  vk.insert(vk.end(), k.alpha1, k.alpha1 + 64);
  vk.insert(vk.end(), k.beta2, k.beta2 + 128);
  vk.insert(vk.end(), k.gamma2, k.gamma2 + 128);
  vk.insert(vk.end(), k.delta2, k.delta2 + 128);
  vk.insert(vk.end(), k.ic, k.ic + (k.l + 1) * 64);
}

// ---- the row-basis extension (OWPR0001) -------------------------------------------------------------------------------------------
// Key material BESIDE an OWPK0001 blob, never inside it: the Lagrange basis of the key's domain at tau in both groups, over the
// QAP rows.  sum_i z_i [a_i(tau)] = sum_j (A z)_j [L_j(tau)], so a prover that holds these points may take the A and B queries
// over the rows instead of the wires (groth16.hip pk_load).  All little-endian:
//   u64 x 4 : magic, n_rows, log_d, 0
//   32 B    : Keccak-256 of the OWPK0001 blob the extension belongs to
//   [L_j(tau)]_1 for j < n_rows (64 B each) | [L_j(tau)]_2 for j < n_rows (128 B each), canonical affine
constexpr uint64_t PR_MAGIC = 0x313030305250574full;  // "OWPR0001"
constexpr size_t PR_HEADER = 32, PR_DIGEST = 32, PR_FIXED = 64;

struct RowsView {
  uint64_t n_rows, log_d;
  const uint8_t *digest, *g1, *g2;  // 32 B | n_rows x 64 B | n_rows x 128 B
};

// structure and ownership: the header agrees with the key's, the length is the one the header implies, the digest is the key's
inline int rows_view(const uint8_t* ext, size_t len, const PkView& pk, const std::string& who, RowsView* v) {
  OG_REQUIRE(len >= PR_FIXED && rd64(ext) == PR_MAGIC, who + ": not an OWPR0001 row-basis extension");
  v->n_rows = rd64(ext + 8);
  v->log_d = rd64(ext + 16);
  OG_REQUIRE(rd64(ext + 24) == 0, who + ": row-basis extension: unknown header word");
  OG_REQUIRE(v->n_rows == pk.n_rows && v->log_d == pk.log_d, who + ": row-basis extension: n_rows / log_d are not the key's");
  OG_REQUIRE(len == PR_FIXED + (size_t)v->n_rows * 192, who + ": row-basis extension: length does not match its header");
  v->digest = ext + PR_HEADER;
  v->g1 = ext + PR_FIXED;
  v->g2 = v->g1 + (size_t)v->n_rows * 64;
  uint8_t want[32];
  keccak256(pk.blob, pk.len, want);
  OG_REQUIRE(memcmp(v->digest, want, 32) == 0, who + ": row-basis extension: the digest is not this key's (another key's extension)");
  return OG_OK;
}

inline void rows_blob(const std::vector<uint8_t>& pk, size_t n_rows, int log_d, const uint8_t* g1, const uint8_t* g2, std::vector<uint8_t>& out) {
  out.clear();
  const uint64_t head[4] = {PR_MAGIC, n_rows, (uint64_t)log_d, 0};
  out.insert(out.end(), (const uint8_t*)head, (const uint8_t*)head + PR_HEADER);
  uint8_t dg[32];
  keccak256(pk.data(), pk.size(), dg);
  out.insert(out.end(), dg, dg + 32);
  out.insert(out.end(), g1, g1 + n_rows * 64);
  out.insert(out.end(), g2, g2 + n_rows * 128);
}

}  // namespace
}  // namespace og
