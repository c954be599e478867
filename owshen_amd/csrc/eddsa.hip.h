// BabyJubJub in projective twisted-Edwards coordinates: what the EdDSA kernels share (eddsa.hip: verification; eddsa_keys.hip:
// decompression, key derivation, signing).  Curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr with a = 168700, d = 168696
// (/root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:174-189); everything is Fr arithmetic on the 9 x 29-bit layer.
#pragma once
#include "field.hip.h"

namespace og {

struct EdPoint {
  Fr x, y, z;
};

// l, the prime order of BASE (251 bits; the curve has 8 l points), as eight words.  Device code reads it at unrolled, constant
// indices only (the form of FrSqrt in eddsa_keys.hip)
struct EdOrder {
  static constexpr int BITS = 251;
  static constexpr uint32_t L[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
};
// word w of l, without dynamic indexing of a constant array
OG_HD uint32_t ed_order_word(int w) {
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) word = k == w ? EdOrder::L[k] : word;
  return word;
}
// bit i of l - 1 (l is odd: only word 0 differs)
OG_HD bool ed_order_minus_1_bit(int i) { return (((ed_order_word(i >> 5) - (i < 32 ? 1u : 0u)) >> (i & 31)) & 1u) != 0; }
// a < l for the eight words of a 256-bit integer, most significant word first
OG_HD bool ed_below_order(const uint32_t a[8]) {
  bool lt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (!decided && a[i] != EdOrder::L[i]) {
      lt = a[i] < EdOrder::L[i];
      decided = true;
    }
  }
  return lt;
}
// a <- a - l on the eight words (a >= l)
OG_HD void ed_sub_order(uint32_t a[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - EdOrder::L[i] - borrow;
    a[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
}

OG_HD Fr ed_const(uint32_t v) { return fe_to_mont(fe_from_u32<FrParams>(v)); }

// unified projective addition on a x^2 + y^2 = 1 + d x^2 y^2 (add-2008-bbjlp: the reference's projective add :118-143 without
// its affine equality test; a is a square and d is not, so the law is complete: it doubles, and the identity is no exception)
__device__ __forceinline__ EdPoint ed_add(const EdPoint& p, const EdPoint& q, const Fr& ca, const Fr& cd) {
  const Fr A = fe_mul(p.z, q.z);
  const Fr B = fe_sqr(A);
  const Fr C = fe_mul(p.x, q.x);
  const Fr D = fe_mul(p.y, q.y);
  const Fr E = fe_mul(cd, fe_mul(C, D));
  const Fr F = fe_sub(B, E);
  const Fr G = fe_add(B, E);
  const Fr t = fe_sub(fe_sub(fe_mul(fe_add(p.x, p.y), fe_add(q.x, q.y)), C), D);
  EdPoint r;
  r.x = fe_mul(fe_mul(A, F), t);
  r.y = fe_mul(fe_mul(A, G), fe_sub(D, fe_mul(ca, C)));
  r.z = fe_mul(F, G);
  return r;
}

OG_HD bool ed_on_curve(const Fr& x, const Fr& y, const Fr& ca, const Fr& cd) {
  const Fr xx = fe_sqr(x), yy = fe_sqr(y);
  return fe_add(fe_mul(ca, xx), yy) == fe_add(Fr::one(), fe_mul(cd, fe_mul(xx, yy)));
}

__device__ __forceinline__ bool canonical_fr(const uint8_t* p) {  // value < r
  const Fr v = fe_load<FrParams>(p);
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) c = ((int32_t)v.l[i] - (int32_t)FrParams::N[i] + c) >> 29;
  return c != 0;  // borrow out: v < N
}

// ---- k * BASE from the window table (built by eddsa_keys.hip k_ed_table, handed out by eddsa_base_table: primitives.h) -------------
constexpr int ED_TAB_WINDOWS = 64, ED_TAB_DIGITS = 16;  // 4-bit windows over 256 bits: scalars range over all of Fr, not only [0, l)
constexpr size_t ED_TAB_BYTES = (size_t)ED_TAB_WINDOWS * ED_TAB_DIGITS * 64;


__device__ __forceinline__ EdPoint ed_identity() {
  EdPoint o;
  o.x = Fr::zero();
  o.y = Fr::one();
  o.z = Fr::one();
  return o;
}

// p0 = k0 BASE and, with TWO, p1 = k1 BASE (the scalars as 8 words each: integers, any value below 2^256), projective.  One rolled
// loop around one addition site; 64 additions per product, the table entry gathered per lane (the table is 64 KiB: it stays in L2).
template <bool TWO>
__device__ __forceinline__ void ed_mul_base(const uint8_t* __restrict__ tab, const uint32_t w0[8], const uint32_t w1[8], EdPoint& p0, EdPoint& p1,
                                            const Fr& ca, const Fr& cd) {
  EdPoint acc = ed_identity();
#pragma unroll 1
  for (int step = 0; step < (TWO ? 2 : 1) * ED_TAB_WINDOWS; step++) {
    const int j = step & (ED_TAB_WINDOWS - 1);
    const bool second = TWO && step >= ED_TAB_WINDOWS;
    if (TWO && step == ED_TAB_WINDOWS) {
      p0 = acc;
      acc = ed_identity();
    }
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) word = k == (j >> 3) ? (second ? w1[k] : w0[k]) : word;
    const uint32_t d = (word >> (4 * (j & 7))) & 15u;
    const uint8_t* e = tab + (size_t)(j * ED_TAB_DIGITS + (int)d) * 64;
    EdPoint q;
    q.x = fe_load<FrParams>(e);
    q.y = fe_load<FrParams>(e + 32);
    q.z = Fr::one();
    acc = ed_add(acc, q, ca, cd);
  }
  if (TWO) p1 = acc;
  else p0 = acc;
}

__device__ __forceinline__ void store_zeros(uint8_t* p, int n16) {
  uint4* q = reinterpret_cast<uint4*>(p);
  for (int k = 0; k < n16; k++) q[k] = make_uint4(0u, 0u, 0u, 0u);
}


}  // namespace og
