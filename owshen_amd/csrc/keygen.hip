// Key material through the C ABI: the withdraw circuit as an R1CS, and Groth16 key generation from
// explicit toxic waste, so that a Rust host needs nothing but libowshen_gpu.so to go from "no key" to proofs.
//
// No reference counterpart (the snapshot's withdraw carries no circuit,
// /root/reference/src/services/api_services/withdraw.rs:27-71).  The statement, its wire order and its row order are
// specified by oracle/py/withdraw.py; owshen_amd/circuit.py holds the same builder on the Python side and the tests
// check all three against each other row by row.  Wire layout is a contract with witness.hip (which fills the wires).
//
//   og_withdraw_r1cs   constraint rows of the depth-D MiMC7 Merkle withdraw circuit (+ synthetic padding gates, + the two
//                      optional density rows), CSR, canonical 32-byte coefficients
//   og_deposit_r1cs / og_split_r1cs / og_join_r1cs / og_transfer_r1cs / og_claim_r1cs / og_send_r1cs / og_redeem_r1cs   the deposit,
//                      the split, the join, the transfer, the claim, the send and the redeem statement, with the same builder
//                      (oracle/py/deposit.py, tests/split_spec.py, tests/join_spec.py, tests/transfer_spec.py, tests/claim_spec.py,
//                      tests/send_spec.py, tests/redeem_spec.py)
//   og_r1cs_from_csr   any R1CS the caller built
//   og_setup           Groth16 key generation from (tau, alpha, beta, gamma, delta): Lagrange evaluations, the three
//                      transposed sparse products, the query scalars and ~3 m + d fixed-base multiplications, all on the
//                      GPU; returns the OWPK0001 / OWVK0001 blobs of include/owshen_gpu.h
#include "ctx.h"
#include "msm.hip.h"
#include "prover.h"
#include "field.hip.h"
#include "keygen.h"
#include "statements.h"
#include "host_fr4.h"
#include "eddsa.hip.h"
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <memory>


namespace og {

// ---- tiny host-side Fr (only what building linear combinations needs: add, small constants, -1) -----------------
struct HFr {
  uint64_t v[4];
};
static const uint64_t FR_MOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};

static HFr hfr_u64(uint64_t x) { return {{x, 0, 0, 0}}; }
static bool hfr_is_zero(const HFr& a) { return (a.v[0] | a.v[1] | a.v[2] | a.v[3]) == 0; }
static bool hfr_ge_mod(const HFr& a) {
  for (int w = 3; w >= 0; w--)
    if (a.v[w] != FR_MOD[w]) return a.v[w] > FR_MOD[w];
  return true;
}
static HFr hfr_add(const HFr& a, const HFr& b) {  // a, b < r
  HFr r;
  unsigned __int128 c = 0;
  for (int w = 0; w < 4; w++) {
    c += (unsigned __int128)a.v[w] + b.v[w];
    r.v[w] = (uint64_t)c;
    c >>= 64;
  }
  if (c || hfr_ge_mod(r)) {
    unsigned __int128 bw = 0;
    for (int w = 0; w < 4; w++) {
      unsigned __int128 d = (unsigned __int128)r.v[w] - FR_MOD[w] - (uint64_t)bw;
      r.v[w] = (uint64_t)d;
      bw = (d >> 64) & 1;
    }
  }
  return r;
}
static HFr hfr_neg_one() { return {{FR_MOD[0] - 1, FR_MOD[1], FR_MOD[2], FR_MOD[3]}}; }
static HFr hfr_from_bytes(const uint8_t* p) {
  HFr r;
  memcpy(r.v, p, 32);
  return r;
}


// ---- BabyJubJub on the host, for the constants of the fixed-base gadget: a x^2 + y^2 = 1 + d x^2 y^2, affine points in the host's
// Montgomery form (host_fr4.h).  Only a doubling is needed: the gadget's constants are 2^i BASE.
struct HEd {
  H4 x, y;
};
static H4 h4_neg(const H4Field& f, const H4& a) { return (a.v[0] | a.v[1] | a.v[2] | a.v[3]) ? h4_sub_raw(f.n, a) : a; }
static H4 h4_sub(const H4Field& f, const H4& a, const H4& b) { return h4_add(f, a, h4_neg(f, b)); }
static H4 h4_small(const H4Field& f, uint64_t v) { return h4_to_mont(f, H4{{v, 0, 0, 0}}); }
static H4 h4_inv(const H4Field& f, const H4& a) {  // a^(r-2), a != 0
  H4 e = f.n, acc = f.one;
  e.v[0] -= 2;  // (r ends in ...0001: no borrow)
  for (int i = 255; i >= 0; i--) {
    acc = h4_mul(f, acc, acc);
    if ((e.v[i >> 6] >> (i & 63)) & 1) acc = h4_mul(f, acc, a);
  }
  return acc;
}
static HFr hfr_of(const H4Field& f, const H4& mont) {
  const H4 c = h4_from_mont(f, mont);
  return {{c.v[0], c.v[1], c.v[2], c.v[3]}};
}
constexpr uint64_t ED_A = 168700, ED_D = 168696;
// BASE (the reference's babyjubjub/mod.rs:177-188; eddsa_keys.hip k_ed_table holds the same words)
static const H4 ED_BASE_X = {{0x2893f3f6bb957051ULL, 0x2ab8d8010534e0b6ULL, 0x4eacb2e09d6277c1ULL, 0x0bb77a6ad63e739bULL}};
static const H4 ED_BASE_Y = {{0x4b3c257a872d7d8bULL, 0xfce0051fb9e13377ULL, 0x25572e1cd16bf9edULL, 0x25797203f7a0b249ULL}};
static HEd hed_double(const H4Field& f, const HEd& p) {  // the complete law with both operands p
  const H4 xx = h4_mul(f, p.x, p.x), yy = h4_mul(f, p.y, p.y), xy = h4_mul(f, p.x, p.y);
  const H4 t = h4_mul(f, h4_small(f, ED_D), h4_mul(f, xx, yy));
  HEd r;
  r.x = h4_mul(f, h4_add(f, xy, xy), h4_inv(f, h4_add(f, f.one, t)));
  r.y = h4_mul(f, h4_sub(f, yy, h4_mul(f, h4_small(f, ED_A), xx)), h4_inv(f, h4_sub(f, f.one, t)));
  return r;
}

typedef std::vector<std::pair<uint32_t, HFr>> LC;  // (wire, coefficient), wires unique, coefficients non-zero

static LC lc_merge(std::initializer_list<const LC*> parts) {
  LC out;
  for (const LC* p : parts)
    for (const auto& t : *p) {
      auto it = std::find_if(out.begin(), out.end(), [&](const std::pair<uint32_t, HFr>& x) { return x.first == t.first; });
      if (it == out.end()) out.push_back(t); else it->second = hfr_add(it->second, t.second);
    }
  out.erase(std::remove_if(out.begin(), out.end(), [](const std::pair<uint32_t, HFr>& x) { return hfr_is_zero(x.second); }), out.end());
  return out;
}

struct R1csBuilder {
  og_r1cs* r;
  uint32_t next = 0;
  const uint8_t* consts;  // 91 x 32 B canonical
  uint32_t alloc(uint32_t n = 1) {
    uint32_t w = next;
    next += n;
    return w;
  }
  void row(int k, const LC& lc) {
    for (const auto& t : lc) {
      r->col[k].push_back(t.first);
      const uint8_t* b = reinterpret_cast<const uint8_t*>(t.second.v);
      r->val[k].insert(r->val[k].end(), b, b + 32);
    }
    r->ptr[k].push_back((uint32_t)r->col[k].size());
  }
  void enforce(const LC& a, const LC& b, const LC& c) {
    row(0, a);
    row(1, b);
    row(2, c);
    r->n_constraints++;
  }
  static LC one(uint32_t w) { return LC{{w, hfr_u64(1)}}; }
  // 91 rounds of x <- (x + k + c_i)^7, four constraints / four wires (t^2, t^4, t^6, t^7) per round
  LC perm(const LC& x_lc, const LC& k_lc) {
    LC cur = x_lc;
    for (int i = 0; i < 91; i++) {
      const LC ci{{0u, hfr_from_bytes(consts + 32 * i)}};
      const LC t = lc_merge({&cur, &k_lc, &ci});
      const uint32_t t2 = alloc(4), t4 = t2 + 1, t6 = t2 + 2, t7 = t2 + 3;
      enforce(t, t, one(t2));
      enforce(one(t2), one(t2), one(t4));
      enforce(one(t4), one(t2), one(t6));
      enforce(one(t6), t, one(t7));
      cur = one(t7);
    }
    return cur;
  }
  // MultiMiMC7([l, r], key 0): k1 = l + E_0(l); out = 2 k1 + r + E_k1(r) ... as two linear rows
  uint32_t hash2(const LC& l_lc, const LC& r_lc, int out_wire = -1) {
    const LC x91 = perm(l_lc, LC{});
    const uint32_t k1 = alloc();
    enforce(lc_merge({&l_lc, &x91}), one(0), one(k1));
    const LC y91 = perm(r_lc, one(k1));
    const uint32_t out = out_wire >= 0 ? (uint32_t)out_wire : alloc();
    const LC k2{{k1, hfr_u64(2)}};
    enforce(lc_merge({&k2, &r_lc, &y91}), one(0), one(out));
    return out;
  }
  // value < 2^128: 128 boolean rows over the wires bits .. bits + 127 (LSB first), then the recomposition row
  void range128(uint32_t value, uint32_t bits) {
    const HFr m1 = hfr_neg_one();
    LC sum;
    for (uint32_t i = 0; i < 128; i++) {
      enforce(one(bits + i), LC{{bits + i, hfr_u64(1)}, {0u, m1}}, LC{});
      HFr p2 = {{0, 0, 0, 0}};
      p2.v[i >> 6] = 1ull << (i & 63);
      sum.push_back({bits + i, p2});
    }
    enforce(sum, one(0), one(value));
  }
  // sum 2^i b_i <= m for the constant m < 2^n_bits over the boolean wires bits .. bits + n_bits - 1 (LSB first), most significant bit
  // first: t starts as the constant 1; a 1-bit of m allocates t' = t b_i (one row), a 0-bit adds the row b_i t = 0.  popcount(m)
  // wires, n_bits rows; the caller makes the wires boolean
  void less_equal_const(uint32_t bits, uint32_t n_bits, const uint64_t m[4]) {
    LC t = one(0);
    for (int i = (int)n_bits - 1; i >= 0; i--) {
      if ((m[i >> 6] >> (i & 63)) & 1) {
        const uint32_t nt = alloc();
        enforce(t, one(bits + i), one(nt));
        t = one(nt);
      } else {
        enforce(one(bits + i), t, LC{});
      }
    }
  }
  // P = (sum 2^i b_i) BASE on BabyJubJub over the wires bits .. bits + n_bits - 1 (LSB first), which it makes boolean.  Per bit the
  // wires w1 = b x1, w2 = b y1, w3 = w1 y1, x3, y3 and six rows: the complete twisted Edwards law with the addend
  // (b u_i, 1 + b (v_i - 1)), (u_i, v_i) = 2^i BASE, on the running sum (x1, y1) that starts at the constants (0, 1).  px, py: the
  // linear combinations of P
  void fixed_base_mul(uint32_t bits, uint32_t n_bits, LC& px, LC& py) {
    const H4Field& f = h4_field();
    const HFr m1 = hfr_neg_one();
    HEd t{h4_to_mont(f, ED_BASE_X), h4_to_mont(f, ED_BASE_Y)};
    LC x1, y1 = one(0);
    for (uint32_t i = 0; i < n_bits; i++) {
      const uint32_t b = bits + i, w1 = alloc(5), w2 = w1 + 1, w3 = w1 + 2, x3 = w1 + 3, y3 = w1 + 4;
      const H4 duv = h4_mul(f, h4_small(f, ED_D), h4_mul(f, t.x, t.y));
      const HFr c_duv = hfr_of(f, duv), c_nduv = hfr_of(f, h4_neg(f, duv)), c_u = hfr_of(f, t.x), c_vm1 = hfr_of(f, h4_sub(f, t.y, f.one));
      const HFr c_nau = hfr_of(f, h4_neg(f, h4_mul(f, h4_small(f, ED_A), t.x)));
      enforce(one(b), LC{{b, hfr_u64(1)}, {0u, m1}}, LC{});
      enforce(one(b), x1, one(w1));
      enforce(one(b), y1, one(w2));
      enforce(one(w1), y1, one(w3));
      const LC tx{{w1, c_vm1}, {w2, c_u}}, ty{{w2, c_vm1}, {w1, c_nau}};
      enforce(one(x3), LC{{0u, hfr_u64(1)}, {w3, c_duv}}, lc_merge({&x1, &tx}));
      enforce(one(y3), LC{{0u, hfr_u64(1)}, {w3, c_nduv}}, lc_merge({&y1, &ty}));
      x1 = one(x3);
      y1 = one(y3);
      t = hed_double(f, t);
    }
    px = x1;
    py = y1;
  }
  // the path from `cur` up to the wire `root`, which is the output wire of the last level's hash: per level a boolean index bit, the
  // `left` selector wire (allocated here) and one hash
  void merkle_walk(uint32_t cur, uint32_t w_sib, uint32_t w_bit, int depth, uint32_t root) {
    const HFr m1 = hfr_neg_one();
    for (int l = 0; l < depth; l++) {
      const uint32_t bit = w_bit + l, s = w_sib + l;
      enforce(one(bit), LC{{bit, hfr_u64(1)}, {0u, m1}}, LC{});              // bit (bit - 1) = 0
      const uint32_t left = alloc();
      enforce(one(bit), LC{{s, hfr_u64(1)}, {cur, m1}}, LC{{left, hfr_u64(1)}, {cur, m1}});  // left = cur + bit (s - cur)
      const LC right{{s, hfr_u64(1)}, {cur, hfr_u64(1)}, {left, m1}};
      cur = hash2(one(left), right, l == depth - 1 ? (int)root : -1);
    }
  }
  // a note is spent: leaf = H(inner = H(nullifier, secret), asset = H(amount, token)), nullifier_hash = H(nullifier, 0) into the
  // wire `nh`, then the leaf's path up to `root`
  void spend_note(uint32_t nullifier, uint32_t secret, uint32_t amount, uint32_t token, uint32_t nh, uint32_t w_sib, uint32_t w_bit, int depth,
                  uint32_t root) {
    const uint32_t inner = hash2(one(nullifier), one(secret));
    const uint32_t asset = hash2(one(amount), one(token));
    const uint32_t leaf = hash2(one(inner), one(asset));
    hash2(one(nullifier), LC{}, (int)nh);
    merkle_walk(leaf, w_sib, w_bit, depth, root);
  }
};

// What every builder with a depth starts and ends with: the statement's shape into r and empty matrices -- `n_pub` is the count the
// builder's wire table is written for --, and, behind the last row, that the rows and wires made are the shape's
static int r1cs_begin(og_r1cs* r, const uint64_t shp[3], uint64_t n_pub, const std::string& who) {
  static const char* const words[] = {"zero", "one", "two", "three", "four", "five", "six", "seven"};
  const std::string count = n_pub < sizeof(words) / sizeof(words[0]) ? std::string(words[n_pub]) : std::to_string(n_pub);
  r->n_wires = shp[0];
  r->n_pub = shp[2];
  for (int k = 0; k < 3; k++) r->ptr[k].assign(1, 0u);
  OG_REQUIRE(r->n_pub == n_pub, who + ": the statement has " + count + " public inputs");
  return OG_OK;
}

constexpr uint32_t KW_ROOT = 1, KW_NH = 2, KW_RECIPIENT = 3, KW_AMOUNT = 4, KW_TOKEN = 5, KW_CHAIN = 6, KW_NULLIFIER = 7, KW_SECRET = 8;
constexpr uint32_t K_PAD_SEGMENT = 64;

static int withdraw_r1cs_build(const uint8_t* mimc_consts, int depth, uint64_t n_pad3, uint64_t n_pad2, int dense, og_r1cs* r) {
  uint64_t shp[3];
  OG_TRY(records_shape_query(ST_WITHDRAW, {depth, n_pad3, n_pad2}, shp));
  OG_REQUIRE(n_pad3 < (1ull << 30) && n_pad2 < (1ull << 30), "og_withdraw_r1cs: too many padding gates");
  OG_TRY(r1cs_begin(r, shp, 6, "og_withdraw_r1cs"));
  R1csBuilder b{r, 0, mimc_consts};
  b.alloc(1 + 6 + 2);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_rsq = b.alloc(), w_csq = b.alloc();
  b.enforce(R1csBuilder::one(KW_RECIPIENT), R1csBuilder::one(KW_RECIPIENT), R1csBuilder::one(w_rsq));
  b.enforce(R1csBuilder::one(KW_CHAIN), R1csBuilder::one(KW_CHAIN), R1csBuilder::one(w_csq));  // binds chain_id to the proof
  b.spend_note(KW_NULLIFIER, KW_SECRET, KW_AMOUNT, KW_TOKEN, KW_NH, w_sib, w_bit, depth, KW_ROOT);
  const uint32_t pad_base = b.next;
  OG_REQUIRE((uint64_t)pad_base + 3 * n_pad3 + 2 * n_pad2 == r->n_wires, "og_withdraw_r1cs: internal wire count mismatch");
  for (uint64_t g = 0; g < n_pad3; g++) {  // (p + 1)(q + 2) = w
    const uint32_t p = pad_base + 3 * (uint32_t)g;
    b.enforce(LC{{p, hfr_u64(1)}, {0u, hfr_u64(1)}}, LC{{p + 1, hfr_u64(1)}, {0u, hfr_u64(2)}}, R1csBuilder::one(p + 2));
  }
  const uint32_t base2 = pad_base + 3 * (uint32_t)n_pad3;
  for (uint64_t g = 0; g < n_pad2; g++) {  // (p + 1)(prev + 2) = w; prev = the previous gate's w, or the constant 1 at a segment start
    const uint32_t p = base2 + 2 * (uint32_t)g, w = p + 1;
    const LC bb = (g % K_PAD_SEGMENT == 0) ? LC{{0u, hfr_u64(3)}} : LC{{w - 2, hfr_u64(1)}, {0u, hfr_u64(2)}};
    b.enforce(LC{{p, hfr_u64(1)}, {0u, hfr_u64(1)}}, bb, R1csBuilder::one(w));
  }
  if (dense) {  // (sum of all wires) * 0 = 0 and 0 * (sum of all wires) = 0: every wire gets an A and a B base
    LC all;
    all.reserve(r->n_wires);
    for (uint32_t w = 0; w < r->n_wires; w++) all.push_back({w, hfr_u64(1)});
    b.enforce(all, LC{}, LC{});
    b.enforce(LC{}, all, LC{});
  }
  OG_REQUIRE(r->n_constraints == shp[1] + (dense ? 2 : 0), "og_withdraw_r1cs: internal constraint count mismatch");
  return OG_OK;
}

// the deposit statement (oracle/py/deposit.py; witness.hip k_deposit_witness): 735 wires, 731 rows
static int deposit_r1cs_build(const uint8_t* mimc_consts, og_r1cs* r) {
  uint64_t shp[3];
  OG_TRY(records_shape_query(ST_DEPOSIT, {}, shp));
  r->n_wires = shp[0];
  r->n_pub = shp[2];
  for (int k = 0; k < 3; k++) r->ptr[k].assign(1, 0u);
  R1csBuilder b{r, 0, mimc_consts};
  constexpr uint32_t DW_COMMITMENT = 1, DW_DEPOSITOR = 2, DW_NULLIFIER = 3, DW_SECRET = 4;
  b.alloc(1 + 2 + 2);
  const uint32_t w_dsq = b.alloc();
  b.enforce(R1csBuilder::one(DW_DEPOSITOR), R1csBuilder::one(DW_DEPOSITOR), R1csBuilder::one(w_dsq));  // binds the depositor to the proof
  b.hash2(R1csBuilder::one(DW_NULLIFIER), R1csBuilder::one(DW_SECRET), (int)DW_COMMITMENT);
  OG_REQUIRE(b.next == r->n_wires && r->n_constraints == shp[1], "og_deposit_r1cs: internal shape mismatch");
  return OG_OK;
}

// ---- the record statements (statements.h): each is its wire table, the rows of its own and calls of the shared gadgets ------------------
// the split statement (tests/split_spec.py; witness.hip k_split_core / k_sw9_*): withdraw part of a note, the rest into a change note
void split_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t SW_ROOT = 1, SW_NH = 2, SW_RECIPIENT = 3, SW_AMOUNT_OUT = 4, SW_TOKEN = 5, SW_CHAIN = 6, SW_CHANGE_LEAF = 7, SW_NULLIFIER = 8,
                     SW_SECRET = 9, SW_AMOUNT = 10, SW_CHANGE_COMMITMENT = 11, SW_CHANGE = 12;
  b.alloc(1 + 7 + 5);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_rsq = b.alloc(), w_csq = b.alloc();
  const uint32_t w_obit = b.alloc(128), w_cbit = b.alloc(128);
  b.enforce(R1csBuilder::one(SW_RECIPIENT), R1csBuilder::one(SW_RECIPIENT), R1csBuilder::one(w_rsq));
  b.enforce(R1csBuilder::one(SW_CHAIN), R1csBuilder::one(SW_CHAIN), R1csBuilder::one(w_csq));
  b.enforce(LC{{SW_AMOUNT_OUT, hfr_u64(1)}, {SW_CHANGE, hfr_u64(1)}}, R1csBuilder::one(0), R1csBuilder::one(SW_AMOUNT));  // amount_out + change = amount
  b.range128(SW_AMOUNT_OUT, w_obit);
  b.range128(SW_CHANGE, w_cbit);
  b.spend_note(SW_NULLIFIER, SW_SECRET, SW_AMOUNT, SW_TOKEN, SW_NH, w_sib, w_bit, depth, SW_ROOT);
  const uint32_t change_asset = b.hash2(R1csBuilder::one(SW_CHANGE), R1csBuilder::one(SW_TOKEN));
  b.hash2(R1csBuilder::one(SW_CHANGE_COMMITMENT), R1csBuilder::one(change_asset), (int)SW_CHANGE_LEAF);
}

// the join statement (tests/join_spec.py; witness.hip k_join_core / k_jw9_*): two notes under one root into one note worth their sum
void join_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t JW_ROOT = 1, JW_NH_A = 2, JW_NH_B = 3, JW_CHAIN = 4, JW_OUT_LEAF = 5, JW_NOTE_A = 6, JW_NOTE_B = 9, JW_TOKEN = 12,
                     JW_OUT_COMMITMENT = 13, JW_SUM = 14, JW_NH_DIFF_INV = 15;  // a note: nullifier, secret, amount
  b.alloc(1 + 5 + 10);
  const uint32_t w_sib = b.alloc(2 * depth), w_bit = b.alloc(2 * depth), w_csq = b.alloc();
  const uint32_t w_bits = b.alloc(3 * 128);
  b.enforce(R1csBuilder::one(JW_CHAIN), R1csBuilder::one(JW_CHAIN), R1csBuilder::one(w_csq));
  b.enforce(LC{{JW_NOTE_A + 2, hfr_u64(1)}, {JW_NOTE_B + 2, hfr_u64(1)}}, R1csBuilder::one(0), R1csBuilder::one(JW_SUM));  // amount_a + amount_b = sum
  b.enforce(LC{{JW_NH_A, hfr_u64(1)}, {JW_NH_B, hfr_neg_one()}}, R1csBuilder::one(JW_NH_DIFF_INV), R1csBuilder::one(0));  // two different notes
  b.range128(JW_NOTE_A + 2, w_bits);
  b.range128(JW_NOTE_B + 2, w_bits + 128);
  b.range128(JW_SUM, w_bits + 256);
  for (int x = 0; x < 2; x++) {  // note a, then note b: both walks end in wire 1
    const uint32_t nt = x ? JW_NOTE_B : JW_NOTE_A;
    b.spend_note(nt, nt + 1, nt + 2, JW_TOKEN, x ? JW_NH_B : JW_NH_A, w_sib + x * depth, w_bit + x * depth, depth, JW_ROOT);
  }
  const uint32_t out_asset = b.hash2(R1csBuilder::one(JW_SUM), R1csBuilder::one(JW_TOKEN));
  b.hash2(R1csBuilder::one(JW_OUT_COMMITMENT), R1csBuilder::one(out_asset), (int)JW_OUT_LEAF);
}

// the transfer statement (tests/transfer_spec.py; witness.hip k_transfer_core / k_tw9_*): part of a note into a leaf for the payee,
// the rest into a change leaf, nothing out of the pool
void transfer_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t TW_ROOT = 1, TW_NH = 2, TW_CHAIN = 3, TW_PAY_LEAF = 4, TW_CHANGE_LEAF = 5, TW_NULLIFIER = 6, TW_SECRET = 7, TW_AMOUNT = 8,
                     TW_TOKEN = 9, TW_PAY_COMMITMENT = 10, TW_PAY_AMOUNT = 11, TW_CHANGE_COMMITMENT = 12, TW_CHANGE = 13;
  b.alloc(1 + 5 + 8);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_csq = b.alloc();
  const uint32_t w_pbit = b.alloc(128), w_cbit = b.alloc(128);
  b.enforce(R1csBuilder::one(TW_CHAIN), R1csBuilder::one(TW_CHAIN), R1csBuilder::one(w_csq));
  b.enforce(LC{{TW_PAY_AMOUNT, hfr_u64(1)}, {TW_CHANGE, hfr_u64(1)}}, R1csBuilder::one(0), R1csBuilder::one(TW_AMOUNT));  // pay_amount + change = amount
  b.range128(TW_PAY_AMOUNT, w_pbit);
  b.range128(TW_CHANGE, w_cbit);
  b.spend_note(TW_NULLIFIER, TW_SECRET, TW_AMOUNT, TW_TOKEN, TW_NH, w_sib, w_bit, depth, TW_ROOT);
  const uint32_t pay_asset = b.hash2(R1csBuilder::one(TW_PAY_AMOUNT), R1csBuilder::one(TW_TOKEN));
  b.hash2(R1csBuilder::one(TW_PAY_COMMITMENT), R1csBuilder::one(pay_asset), (int)TW_PAY_LEAF);
  const uint32_t change_asset = b.hash2(R1csBuilder::one(TW_CHANGE), R1csBuilder::one(TW_TOKEN));
  b.hash2(R1csBuilder::one(TW_CHANGE_COMMITMENT), R1csBuilder::one(change_asset), (int)TW_CHANGE_LEAF);
}

// the claim statement (tests/claim_spec.py; witness.hip k_claim_core): an owned note, bound to the one-time key P = x BASE, into an
// ordinary note of the same value
void claim_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t CW_ROOT = 1, CW_NH = 2, CW_CHAIN = 3, CW_OUT_LEAF = 4, CW_X = 5, CW_AMOUNT = 6, CW_TOKEN = 7, CW_OUT_COMMITMENT = 8;
  constexpr uint32_t C_BITS = EdOrder::BITS;
  b.alloc(1 + 4 + 4);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_csq = b.alloc();
  const uint32_t w_xbit = b.alloc(C_BITS);
  b.enforce(R1csBuilder::one(CW_CHAIN), R1csBuilder::one(CW_CHAIN), R1csBuilder::one(w_csq));
  LC sum;
  for (uint32_t i = 0; i < C_BITS; i++) {
    HFr p2 = {{0, 0, 0, 0}};
    p2.v[i >> 6] = 1ull << (i & 63);
    sum.push_back({w_xbit + i, p2});
  }
  b.enforce(sum, R1csBuilder::one(0), R1csBuilder::one(CW_X));  // x = sum 2^i b_i
  b.enforce(R1csBuilder::one(0), R1csBuilder::one(0), R1csBuilder::one(0));
  uint64_t l_minus_1[4];  // (l is odd)
  for (int k = 0; k < 4; k++) l_minus_1[k] = (uint64_t)EdOrder::L[2 * k] | (uint64_t)EdOrder::L[2 * k + 1] << 32;
  l_minus_1[0] -= 1;
  b.less_equal_const(w_xbit, C_BITS, l_minus_1);  // x < l: without it x + l is a second key for the same note
  LC px, py;
  b.fixed_base_mul(w_xbit, C_BITS, px, py);
  const uint32_t c = b.hash2(px, py);
  const uint32_t asset = b.hash2(R1csBuilder::one(CW_AMOUNT), R1csBuilder::one(CW_TOKEN));
  const uint32_t leaf = b.hash2(R1csBuilder::one(c), R1csBuilder::one(asset));
  b.hash2(R1csBuilder::one(CW_X), R1csBuilder::one(0), (int)CW_NH);  // H(x, 1): an ordinary spend publishes H(nullifier, 0)
  b.merkle_walk(leaf, w_sib, w_bit, depth, CW_ROOT);
  b.hash2(R1csBuilder::one(CW_OUT_COMMITMENT), R1csBuilder::one(asset), (int)CW_OUT_LEAF);  // the SAME asset wire
}

// the rows send and redeem share behind their own first rows (claim keeps its own text: a one * one row follows its recomposition):
// x = sum 2^i b_i, x < l, P = x BASE, then the gadgets c, asset, leaf, nullifier_hash = H(x, 1) and the path
static void owned_front_rows(R1csBuilder& b, uint32_t w_x, uint32_t w_amount, uint32_t w_token, uint32_t w_nh, uint32_t w_xbit, uint32_t w_sib,
                             uint32_t w_bit, int depth, uint32_t w_root) {
  constexpr uint32_t C_BITS = EdOrder::BITS;
  LC sum;
  for (uint32_t i = 0; i < C_BITS; i++) {
    HFr p2 = {{0, 0, 0, 0}};
    p2.v[i >> 6] = 1ull << (i & 63);
    sum.push_back({w_xbit + i, p2});
  }
  b.enforce(sum, R1csBuilder::one(0), R1csBuilder::one(w_x));
  uint64_t l_minus_1[4];  // (l is odd)
  for (int k = 0; k < 4; k++) l_minus_1[k] = (uint64_t)EdOrder::L[2 * k] | (uint64_t)EdOrder::L[2 * k + 1] << 32;
  l_minus_1[0] -= 1;
  b.less_equal_const(w_xbit, C_BITS, l_minus_1);
  LC px, py;
  b.fixed_base_mul(w_xbit, C_BITS, px, py);
  const uint32_t c = b.hash2(px, py);
  const uint32_t asset = b.hash2(R1csBuilder::one(w_amount), R1csBuilder::one(w_token));
  const uint32_t leaf = b.hash2(R1csBuilder::one(c), R1csBuilder::one(asset));
  b.hash2(R1csBuilder::one(w_x), R1csBuilder::one(0), (int)w_nh);  // H(x, 1), as claim: one spent set for the three owned statements
  b.merkle_walk(leaf, w_sib, w_bit, depth, w_root);
}

// the send statement (tests/send_spec.py; witness.hip k_send_core): transfer for an owned note
void send_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t NW_ROOT = 1, NW_NH = 2, NW_CHAIN = 3, NW_PAY_LEAF = 4, NW_CHANGE_LEAF = 5, NW_X = 6, NW_AMOUNT = 7, NW_TOKEN = 8,
                     NW_PAY_COMMITMENT = 9, NW_PAY_AMOUNT = 10, NW_CHANGE_COMMITMENT = 11, NW_CHANGE = 12;
  b.alloc(1 + 5 + 7);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_csq = b.alloc();
  const uint32_t w_pbit = b.alloc(128), w_cbit = b.alloc(128), w_xbit = b.alloc(EdOrder::BITS);
  b.enforce(R1csBuilder::one(NW_CHAIN), R1csBuilder::one(NW_CHAIN), R1csBuilder::one(w_csq));
  b.enforce(LC{{NW_PAY_AMOUNT, hfr_u64(1)}, {NW_CHANGE, hfr_u64(1)}}, R1csBuilder::one(0), R1csBuilder::one(NW_AMOUNT));  // pay_amount + change = amount
  b.range128(NW_PAY_AMOUNT, w_pbit);
  b.range128(NW_CHANGE, w_cbit);
  owned_front_rows(b, NW_X, NW_AMOUNT, NW_TOKEN, NW_NH, w_xbit, w_sib, w_bit, depth, NW_ROOT);
  const uint32_t pay_asset = b.hash2(R1csBuilder::one(NW_PAY_AMOUNT), R1csBuilder::one(NW_TOKEN));
  b.hash2(R1csBuilder::one(NW_PAY_COMMITMENT), R1csBuilder::one(pay_asset), (int)NW_PAY_LEAF);
  const uint32_t change_asset = b.hash2(R1csBuilder::one(NW_CHANGE), R1csBuilder::one(NW_TOKEN));  // the ONE token wire
  b.hash2(R1csBuilder::one(NW_CHANGE_COMMITMENT), R1csBuilder::one(change_asset), (int)NW_CHANGE_LEAF);
}

// the redeem statement (tests/redeem_spec.py; witness.hip k_redeem_core): split for an owned note
void redeem_r1cs_rows(R1csBuilder& b, int depth) {
  constexpr uint32_t EW_ROOT = 1, EW_NH = 2, EW_RECIPIENT = 3, EW_AMOUNT_OUT = 4, EW_TOKEN = 5, EW_CHAIN = 6, EW_CHANGE_LEAF = 7, EW_X = 8,
                     EW_AMOUNT = 9, EW_CHANGE_COMMITMENT = 10, EW_CHANGE = 11;
  b.alloc(1 + 7 + 4);
  const uint32_t w_sib = b.alloc(depth), w_bit = b.alloc(depth), w_rsq = b.alloc(), w_csq = b.alloc();
  const uint32_t w_obit = b.alloc(128), w_cbit = b.alloc(128), w_xbit = b.alloc(EdOrder::BITS);
  b.enforce(R1csBuilder::one(EW_RECIPIENT), R1csBuilder::one(EW_RECIPIENT), R1csBuilder::one(w_rsq));
  b.enforce(R1csBuilder::one(EW_CHAIN), R1csBuilder::one(EW_CHAIN), R1csBuilder::one(w_csq));
  b.enforce(LC{{EW_AMOUNT_OUT, hfr_u64(1)}, {EW_CHANGE, hfr_u64(1)}}, R1csBuilder::one(0), R1csBuilder::one(EW_AMOUNT));  // amount_out + change = amount
  b.range128(EW_AMOUNT_OUT, w_obit);
  b.range128(EW_CHANGE, w_cbit);
  owned_front_rows(b, EW_X, EW_AMOUNT, EW_TOKEN, EW_NH, w_xbit, w_sib, w_bit, depth, EW_ROOT);
  const uint32_t change_asset = b.hash2(R1csBuilder::one(EW_CHANGE), R1csBuilder::one(EW_TOKEN));
  b.hash2(R1csBuilder::one(EW_CHANGE_COMMITMENT), R1csBuilder::one(change_asset), (int)EW_CHANGE_LEAF);
}

static int records_r1cs_build(const Statement& st, const uint8_t* mimc_consts, int depth, og_r1cs* r) {
  const std::string who = "og_" + std::string(st.name) + "_r1cs";
  uint64_t shp[3];
  OG_TRY(records_shape_query(st, {depth}, shp));
  OG_TRY(r1cs_begin(r, shp, (uint64_t)st.n_pub, who));
  R1csBuilder b{r, 0, mimc_consts};
  st.r1cs_rows(b, depth);
  OG_REQUIRE(b.next == r->n_wires && r->n_constraints == shp[1], who + ": internal shape mismatch");
  return OG_OK;
}

// ---- setup kernels ---------------------------------------------------------------------------------------------
// toxic: tau | alpha | beta | gamma | delta (canonical).  out: 0 zt = tau^d - 1, 1 1/gamma, 2 1/delta, 3 zt/delta
__global__ void k_setup_scalars(const uint8_t* __restrict__ toxic, int log_d, uint8_t* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Fr tau = fe_to_mont(fe_load<FrParams>(toxic));
  Fr zt = tau;
  for (int i = 0; i < log_d; i++) zt = fe_sqr(zt);
  zt = fe_sub(zt, Fr::one());
  const Fr ginv = fe_inv(fe_to_mont(fe_load<FrParams>(toxic + 96)));
  const Fr dinv = fe_inv(fe_to_mont(fe_load<FrParams>(toxic + 128)));
  fe_store(out, fe_from_mont(zt));
  fe_store(out + 32, fe_from_mont(ginv));
  fe_store(out + 64, fe_from_mont(dinv));
  fe_store(out + 96, fe_from_mont(fe_mul(zt, dinv)));
}

// kk_i = beta a_i + alpha b_i + c_i;  i <= n_pub: ic[i] = kk_i / gamma, else l[i - n_pub - 1] = kk_i / delta  (all canonical)
__global__ void __launch_bounds__(256) k_setup_kk(const uint8_t* __restrict__ at_a, const uint8_t* __restrict__ at_b, const uint8_t* __restrict__ at_c,
                                                 const uint8_t* __restrict__ toxic, const uint8_t* __restrict__ derived, size_t m, size_t n_pub,
                                                 uint8_t* __restrict__ ic, uint8_t* __restrict__ l) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Fr alpha = fe_to_mont(fe_load<FrParams>(toxic + 32)), beta = fe_to_mont(fe_load<FrParams>(toxic + 64));
  const Fr a = fe_to_mont(fe_load<FrParams>(at_a + i * 32)), b = fe_to_mont(fe_load<FrParams>(at_b + i * 32));
  const Fr c = fe_to_mont(fe_load<FrParams>(at_c + i * 32));
  const Fr kk = fe_add(fe_add(fe_mul(beta, a), fe_mul(alpha, b)), c);
  if (i <= n_pub)
    fe_store(ic + i * 32, fe_from_mont(fe_mul(kk, fe_to_mont(fe_load<FrParams>(derived + 32)))));
  else
    fe_store(l + (i - n_pub - 1) * 32, fe_from_mont(fe_mul(kk, fe_to_mont(fe_load<FrParams>(derived + 64)))));
}

// out[j] = (zt / delta) tau^j, canonical
__global__ void __launch_bounds__(256) k_setup_h(const uint8_t* __restrict__ toxic, const uint8_t* __restrict__ derived, size_t n,
                                                uint8_t* __restrict__ out) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  Fr b = fe_to_mont(fe_load<FrParams>(toxic));
  Fr acc = fe_to_mont(fe_load<FrParams>(derived + 96));
  for (size_t e = j; e; e >>= 1) {
    if (e & 1) acc = fe_mul(acc, b);
    b = fe_sqr(b);
  }
  fe_store(out + j * 32, fe_from_mont(acc));
}

extern const uint8_t G1_GEN_BYTES[64] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                         2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// the EIP-197 G2 generator: x.c0 | x.c1 | y.c0 | y.c1, 32-byte little-endian each
extern const uint8_t G2_GEN_BYTES[128] = {
    0xed, 0xf6, 0x92, 0xd9, 0x5c, 0xbd, 0xde, 0x46, 0xdd, 0xda, 0x5e, 0xf7, 0xd4, 0x22, 0x43, 0x67, 0x79, 0x44, 0x5c, 0x5e, 0x66, 0x00,
    0x6a, 0x42, 0x76, 0x1e, 0x1f, 0x12, 0xef, 0xde, 0x00, 0x18, 0xc2, 0x12, 0xf3, 0xae, 0xb7, 0x85, 0xe4, 0x97, 0x12, 0xe7, 0xa9, 0x35,
    0x33, 0x49, 0xaa, 0xf1, 0x25, 0x5d, 0xfb, 0x31, 0xb7, 0xbf, 0x60, 0x72, 0x3a, 0x48, 0x0d, 0x92, 0x93, 0x93, 0x8e, 0x19, 0xaa, 0x7d,
    0xfa, 0x66, 0x01, 0xcc, 0xe6, 0x4c, 0x7b, 0xd3, 0x43, 0x0c, 0x69, 0xe7, 0xd1, 0xe3, 0x8f, 0x40, 0xcb, 0x8d, 0x80, 0x71, 0xab, 0x4a,
    0xeb, 0x6d, 0x8c, 0xdb, 0xa5, 0x5e, 0xc8, 0x12, 0x5b, 0x97, 0x22, 0xd1, 0xdc, 0xda, 0xac, 0x55, 0xf3, 0x8e, 0xb3, 0x70, 0x33, 0x31,
    0x4b, 0xbc, 0x95, 0x33, 0x0c, 0x69, 0xad, 0x99, 0x9e, 0xec, 0x75, 0xf0, 0x5f, 0x58, 0xd0, 0x89, 0x06, 0x09};

struct DevBuf {  // hipMalloc'd scratch released on every exit path
  std::vector<void*> ptrs;
  ~DevBuf() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  int get(size_t bytes, uint8_t** out) {
    void* p = nullptr;
    OG_HIP(hipMalloc(&p, bytes ? bytes : 32));
    ptrs.push_back(p);
    *out = static_cast<uint8_t*>(p);
    return OG_OK;
  }
};

// the QAP rows of a circuit: its constraints, then the input-consistency rows A = wire i for i <= n_pub (B = C = 0)
int r1cs_qap_rows(const og_r1cs* r, const std::string& who, QapRows* out) {
  const size_t m = r->n_wires, l = r->n_pub, nc = r->n_constraints;
  OG_REQUIRE(m >= 1 && l < m && m < (1ull << 31), who + ": bad wire counts");
  for (int k = 0; k < 3; k++) {
    OG_REQUIRE(r->ptr[k].size() == nc + 1 && r->ptr[k][0] == 0 && r->ptr[k][nc] == r->col[k].size() && r->val[k].size() == r->col[k].size() * 32,
               who + ": malformed R1CS");
    for (uint32_t c : r->col[k]) OG_REQUIRE(c < m, who + ": R1CS column out of range");
  }
  const uint8_t one32[32] = {1};
  for (int k = 0; k < 3; k++) {
    out->ptr[k] = r->ptr[k];
    out->col[k] = r->col[k];
    out->val[k] = r->val[k];
    for (size_t i = 0; i <= l; i++) {
      if (k == 0) {
        out->col[k].push_back((uint32_t)i);
        out->val[k].insert(out->val[k].end(), one32, one32 + 32);
      }
      out->ptr[k].push_back((uint32_t)out->col[k].size());
    }
    OG_REQUIRE(out->col[k].size() < (1ull << 32), who + ": nnz too large");
  }
  return OG_OK;
}

// CSR over n_rows rows -> CSR of the transpose over m columns (tcol holds ROWS; entries of a column keep their row order)
void csr_transpose(const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& col, const std::vector<uint8_t>& val, size_t n_rows, size_t m,
                   std::vector<uint32_t>& tptr, std::vector<uint32_t>& tcol, std::vector<uint8_t>& tval) {
  const size_t nnz = col.size();
  tptr.assign(m + 1, 0);
  tcol.resize(nnz);
  tval.resize(nnz * 32);
  for (uint32_t c : col) tptr[c + 1]++;
  for (size_t i = 0; i < m; i++) tptr[i + 1] += tptr[i];
  std::vector<uint32_t> cursor(tptr.begin(), tptr.end() - 1);
  for (size_t row = 0; row < n_rows; row++)
    for (uint32_t e = ptr[row]; e < ptr[row + 1]; e++) {
      const uint32_t pos = cursor[col[e]]++;
      tcol[pos] = (uint32_t)row;
      memcpy(&tval[(size_t)pos * 32], &val[(size_t)e * 32], 32);
    }
}

// rows_ext (optional): the OWPR0001 row-basis extension of the key (key_blob.h), left EMPTY when neither the A nor the B query
// of this circuit would run over the rows (row_form_pays, the rule pk_load applies): then the points are never read
static int keygen_setup(og_ctx* ctx, const og_r1cs* r, const uint8_t toxic[160], std::vector<uint8_t>& pk, std::vector<uint8_t>& vk,
                        std::vector<uint8_t>* rows_ext = nullptr) {
  const size_t m = r->n_wires, l = r->n_pub, nc = r->n_constraints, n_rows = nc + l + 1;
  QapRows rows;
  OG_TRY(r1cs_qap_rows(r, "og_setup", &rows));
  int log_d = 1;
  while (((size_t)1 << log_d) < n_rows) log_d++;
  OG_REQUIRE(log_d <= 28, "og_setup: too many constraints for the 2^28 domain");
  const size_t d = (size_t)1 << log_d, nl = m - l - 1, nh = d - 1;
  for (int k = 0; k < 5; k++) {
    const HFr t = hfr_from_bytes(toxic + 32 * k);
    OG_REQUIRE(!hfr_is_zero(t) && !hfr_ge_mod(t), "og_setup: toxic values must be canonical and non-zero");
  }
  DevBuf dev;
  uint8_t *toxic_d, *derived_d, *lag_d, *at_d[3], *ic_s, *l_s, *h_s;
  OG_TRY(dev.get(160, &toxic_d));
  OG_TRY(dev.get(128, &derived_d));
  OG_TRY(dev.get(d * 32, &lag_d));
  for (int k = 0; k < 3; k++) OG_TRY(dev.get(m * 32, &at_d[k]));
  OG_TRY(dev.get((l + 1) * 32, &ic_s));
  OG_TRY(dev.get(nl * 32, &l_s));
  OG_TRY(dev.get(nh * 32, &h_s));
  OG_HIP(hipMemcpyAsync(toxic_d, toxic, 160, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_setup_scalars, dim3(1), dim3(64), 0, ctx->stream, toxic_d, log_d, derived_d);
  OG_HIP(hipGetLastError());
  uint8_t derived[128];
  OG_HIP(hipMemcpyAsync(derived, derived_d, 128, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  OG_REQUIRE(!hfr_is_zero(hfr_from_bytes(derived)), "og_setup: tau lies in the evaluation domain");
  OG_TRY(lagrange_evals(ctx, log_d, toxic, lag_d));
  // a_i(tau) = sum_rows M[row][i] L_row(tau): the transposed sparse product (QAP rows = constraints, then the
  // input-consistency rows A = wire i for i <= n_pub)
  for (int k = 0; k < 3; k++) {
    const size_t nnz = rows.col[k].size();
    std::vector<uint32_t> tptr, tcol;
    std::vector<uint8_t> tval;
    csr_transpose(rows.ptr[k], rows.col[k], rows.val[k], n_rows, m, tptr, tcol, tval);
    uint8_t *p_d, *c_d, *v_d;
    OG_TRY(dev.get((m + 1) * 4, &p_d));
    OG_TRY(dev.get(nnz * 4, &c_d));
    OG_TRY(dev.get(nnz * 32, &v_d));
    OG_HIP(hipMemcpyAsync(p_d, tptr.data(), (m + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(c_d, tcol.data(), nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(v_d, tval.data(), nnz * 32, hipMemcpyHostToDevice, ctx->stream));
    OG_TRY(spmv_canonical(ctx, (const uint32_t*)p_d, (const uint32_t*)c_d, v_d, m, lag_d, at_d[k]));
    OG_HIP(hipStreamSynchronize(ctx->stream));  // the host staging vectors die at the end of this iteration
  }
  hipLaunchKernelGGL(k_setup_kk, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, at_d[0], at_d[1], at_d[2], toxic_d, derived_d, m, l, ic_s, l_s);
  OG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_setup_h, dim3(grid_for(nh, 256)), dim3(256), 0, ctx->stream, toxic_d, derived_d, nh, h_s);
  OG_HIP(hipGetLastError());
  // fixed-base multiplications: the five queries, IC, and the constants (alpha, beta, gamma, delta) in both groups
  struct Job { int is_g2; const uint8_t* sc; size_t n; std::vector<uint8_t> out; };
  Job jobs[8] = {{0, at_d[0], m, {}}, {0, at_d[1], m, {}}, {1, at_d[1], m, {}}, {0, l_s, nl, {}}, {0, h_s, nh, {}},
                 {0, ic_s, l + 1, {}}, {0, toxic_d + 32, 4, {}}, {1, toxic_d + 32, 4, {}}};
  uint8_t* pts_d;
  OG_TRY(dev.get(std::max<size_t>(std::max<size_t>(std::max<size_t>(m * 128, nh * 64), n_rows * 128), 512), &pts_d));
  for (Job& j : jobs) {
    const size_t pb = j.is_g2 ? 128 : 64;
    j.out.resize(j.n * pb);
    if (j.n == 0) continue;
    OG_TRY(scalar_mul_fixed(ctx, j.is_g2, j.is_g2 ? G2_GEN_BYTES : G1_GEN_BYTES, j.sc, j.n, pts_d));  // synchronises
    OG_HIP(hipMemcpyAsync(j.out.data(), pts_d, j.n * pb, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
  }
  const std::vector<uint8_t>&c1 = jobs[6].out, &c2 = jobs[7].out;  // index 0 alpha, 1 beta, 2 gamma, 3 delta
  KeyParts parts;
  parts.m = m; parts.l = l; parts.log_d = log_d; parts.n_rows = n_rows;
  parts.alpha1 = &c1[0]; parts.beta1 = &c1[64]; parts.delta1 = &c1[192];
  parts.beta2 = &c2[128]; parts.gamma2 = &c2[256]; parts.delta2 = &c2[384];
  for (int q = 0; q < 5; q++) parts.query[q] = jobs[q].out.data();
  parts.ic = jobs[5].out.data();
  key_blobs(parts, rows, pk, vk);
  if (rows_ext) {
    rows_ext->clear();
    bool pays = OG_HOOK_INT("OG_ROW_FORM", -1) == 1;  // (hooks builds: the form pk_load can then be forced into)
    for (int k = 0; k < 2; k++) {  // A | B: rows with an entry against wires with one
      std::vector<uint8_t> seen(m, 0);
      size_t rows_q = 0, wires_q = 0;
      for (size_t row = 0; row < n_rows; row++) rows_q += rows.ptr[k][row + 1] > rows.ptr[k][row];
      for (uint32_t c : rows.col[k]) wires_q += !seen[c]++;
      pays = pays || row_form_pays(rows_q, wires_q);
    }
    if (pays) {  // [L_j(tau)] in both groups: the Lagrange evaluations are still in lag_d
      std::vector<uint8_t> g1(n_rows * 64), g2(n_rows * 128);
      OG_TRY(scalar_mul_fixed(ctx, 0, G1_GEN_BYTES, lag_d, n_rows, pts_d));  // synchronises
      OG_HIP(hipMemcpy(g1.data(), pts_d, g1.size(), hipMemcpyDeviceToHost));
      OG_TRY(scalar_mul_fixed(ctx, 1, G2_GEN_BYTES, lag_d, n_rows, pts_d));
      OG_HIP(hipMemcpy(g2.data(), pts_d, g2.size(), hipMemcpyDeviceToHost));
      rows_blob(pk, n_rows, log_d, g1.data(), g2.data(), *rows_ext);
    }
  }
  return OG_OK;
}

}  // namespace og

using namespace og;

// the body behind og_<statement>_r1cs of the record statements (statements.h)
static int record_r1cs(const Statement& st, og_ctx* ctx, int depth, og_r1cs** out) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx != nullptr && out != nullptr, "og_" + std::string(st.name) + "_r1cs: null argument");
    *out = nullptr;
    og_r1cs* r = new og_r1cs();
    int rc = records_r1cs_build(st, ctx->mimc_consts_canon, depth, r);
    if (rc != OG_OK) {
      delete r;
      return rc;
    }
    *out = r;
    return OG_OK;
  });
}

extern "C" {

int og_withdraw_r1cs(og_ctx* ctx, int depth, uint64_t n_pad3, uint64_t n_pad2, int dense, og_r1cs** out) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx != nullptr && out != nullptr, "og_withdraw_r1cs: null argument");
    *out = nullptr;
    og_r1cs* r = new og_r1cs();
    int rc = withdraw_r1cs_build(ctx->mimc_consts_canon, depth, n_pad3, n_pad2, dense, r);
    if (rc != OG_OK) {
      delete r;
      return rc;
    }
    *out = r;
    return OG_OK;
  });
}

int og_deposit_r1cs(og_ctx* ctx, og_r1cs** out) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx != nullptr && out != nullptr, "og_deposit_r1cs: null argument");
    *out = nullptr;
    og_r1cs* r = new og_r1cs();
    int rc = deposit_r1cs_build(ctx->mimc_consts_canon, r);
    if (rc != OG_OK) {
      delete r;
      return rc;
    }
    *out = r;
    return OG_OK;
  });
}

int og_split_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_SPLIT, ctx, depth, out); }
int og_join_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_JOIN, ctx, depth, out); }
int og_transfer_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_TRANSFER, ctx, depth, out); }
int og_claim_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_CLAIM, ctx, depth, out); }
int og_send_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_SEND, ctx, depth, out); }
int og_redeem_r1cs(og_ctx* ctx, int depth, og_r1cs** out) { return record_r1cs(ST_REDEEM, ctx, depth, out); }

int og_r1cs_from_csr(uint64_t n_wires, uint64_t n_pub, uint64_t n_constraints, const uint32_t* const ptr[3], const uint32_t* const col[3],
                     const uint8_t* const val[3], og_r1cs** out) {
  return guarded([&]() -> int {
    OG_REQUIRE(out != nullptr && ptr && col && val, "og_r1cs_from_csr: null argument");
    *out = nullptr;
    OG_REQUIRE(n_wires >= 1 && n_pub < n_wires && n_wires < (1ull << 31) && n_constraints < (1ull << 31), "og_r1cs_from_csr: bad sizes");
    std::unique_ptr<og_r1cs> r(new og_r1cs());
    r->n_wires = n_wires; r->n_pub = n_pub; r->n_constraints = n_constraints;
    for (int k = 0; k < 3; k++) {
      OG_REQUIRE(ptr[k] != nullptr, "og_r1cs_from_csr: null row pointers");
      OG_REQUIRE(ptr[k][0] == 0, "og_r1cs_from_csr: row pointers must start at 0");
      for (uint64_t i = 0; i < n_constraints; i++) OG_REQUIRE(ptr[k][i] <= ptr[k][i + 1], "og_r1cs_from_csr: row pointers not monotone");
      const size_t nnz = ptr[k][n_constraints];
      OG_REQUIRE(nnz == 0 || (col[k] && val[k]), "og_r1cs_from_csr: null columns / values");
      r->ptr[k].assign(ptr[k], ptr[k] + n_constraints + 1);
      r->col[k].assign(col[k], col[k] + nnz);
      r->val[k].assign(val[k], val[k] + nnz * 32);
      for (uint32_t c : r->col[k]) OG_REQUIRE(c < n_wires, "og_r1cs_from_csr: column out of range");
    }
    *out = r.release();
    return OG_OK;
  });
}

void og_r1cs_free(og_r1cs* r) { delete r; }

int og_r1cs_info(const og_r1cs* r, uint64_t info[6]) {
  return guarded([&]() -> int {
    OG_REQUIRE(r != nullptr && info != nullptr, "og_r1cs_info: null argument");
    info[0] = r->n_wires; info[1] = r->n_pub; info[2] = r->n_constraints;
    for (int k = 0; k < 3; k++) info[3 + k] = r->col[k].size();
    return OG_OK;
  });
}

int og_r1cs_export(const og_r1cs* r, int matrix, uint32_t* ptr_out, uint32_t* col_out, uint8_t* val_out) {
  return guarded([&]() -> int {
    OG_REQUIRE(r != nullptr && matrix >= 0 && matrix < 3 && ptr_out != nullptr, "og_r1cs_export: bad arguments");
    memcpy(ptr_out, r->ptr[matrix].data(), r->ptr[matrix].size() * 4);
    if (!r->col[matrix].empty()) {
      OG_REQUIRE(col_out != nullptr && val_out != nullptr, "og_r1cs_export: null output");
      memcpy(col_out, r->col[matrix].data(), r->col[matrix].size() * 4);
      memcpy(val_out, r->val[matrix].data(), r->val[matrix].size());
    }
    return OG_OK;
  });
}

static int setup_entry(const char* who, og_ctx* ctx, const og_r1cs* r1cs, const uint8_t toxic[160], uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out,
                       size_t* vk_len, uint8_t** rows_out, size_t* rows_len) {
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && r1cs && toxic && pk_out && pk_len && vk_out && vk_len, std::string(who) + ": null argument");
    *pk_out = *vk_out = nullptr;
    *pk_len = *vk_len = 0;
    if (rows_out) { *rows_out = nullptr; *rows_len = 0; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    std::vector<uint8_t> pk, vk, ext;
    OG_TRY(keygen_setup(ctx, r1cs, toxic, pk, vk, rows_out ? &ext : nullptr));
    uint8_t* a = static_cast<uint8_t*>(malloc(pk.size() ? pk.size() : 1));
    uint8_t* b = static_cast<uint8_t*>(malloc(vk.size() ? vk.size() : 1));
    uint8_t* e = ext.empty() ? nullptr : static_cast<uint8_t*>(malloc(ext.size()));
    if (!a || !b || (!ext.empty() && !e)) {
      free(a);
      free(b);
      free(e);
      set_error(std::string(who) + ": out of host memory");
      return OG_ERR_INVALID;
    }
    memcpy(a, pk.data(), pk.size());
    memcpy(b, vk.data(), vk.size());
    if (e) memcpy(e, ext.data(), ext.size());
    *pk_out = a; *pk_len = pk.size();
    *vk_out = b; *vk_len = vk.size();
    if (rows_out) { *rows_out = e; *rows_len = ext.size(); }
    return OG_OK;
  });
}

int og_setup(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t toxic[160], uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out, size_t* vk_len) {
  return setup_entry("og_setup", ctx, r1cs, toxic, pk_out, pk_len, vk_out, vk_len, nullptr, nullptr);
}

int og_setup_rows(og_ctx* ctx, const og_r1cs* r1cs, const uint8_t toxic[160], uint8_t** pk_out, size_t* pk_len, uint8_t** vk_out, size_t* vk_len,
                  uint8_t** rows_out, size_t* rows_len) {
  if (!rows_out || !rows_len) {
    set_error("og_setup_rows: null argument");
    return OG_ERR_INVALID;
  }
  return setup_entry("og_setup_rows", ctx, r1cs, toxic, pk_out, pk_len, vk_out, vk_len, rows_out, rows_len);
}

void og_blob_free(uint8_t* blob) { free(blob); }

}  // extern "C"
