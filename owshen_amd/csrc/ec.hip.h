// BN254 G1 / G2 group law for gfx950.  No reference counterpart
// (the snapshot has no G1/G2); curves per EIP-196/197:
//   G1: y^2 = x^3 + 3 over Fq;   G2: y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1).
// Accumulators use extended Jacobian "XYZZ" coordinates (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2):
// mixed add 8M+2S, full add 12M+2S, double 6M+3S (EFD madd-2008-s / add-2008-s / dbl-2008-s-1),
// which minimises Montgomery multiplications -- the binding resource on CDNA4.
// Affine infinity is encoded as (0, 0) (not on either curve); XYZZ infinity as ZZ = 0.
#pragma once
#include "field.hip.h"

namespace og {

// ---- Fq2 --------------------------------------------------------------------
struct Fq2 {
  Fq c0, c1;
  OG_HD static Fq2 zero() { return {Fq::zero(), Fq::zero()}; }
  OG_HD static Fq2 one() { return {Fq::one(), Fq::zero()}; }
  OG_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  OG_HD bool operator==(const Fq2& b) const { return c0 == b.c0 && c1 == b.c1; }
};

// uniform field interface so the group law is written once
OG_HD Fq f_add(const Fq& a, const Fq& b) { return fe_add(a, b); }
OG_HD Fq f_sub(const Fq& a, const Fq& b) { return fe_sub(a, b); }
OG_HD Fq f_mul(const Fq& a, const Fq& b) { return fe_mul(a, b); }
OG_HD Fq f_sqr(const Fq& a) { return fe_sqr(a); }
OG_HD Fq f_dbl(const Fq& a) { return fe_dbl(a); }
OG_HD Fq f_neg(const Fq& a) { return fe_neg(a); }
OG_HD Fq f_inv(const Fq& a) { return fe_inv(a); }

OG_HD Fq2 f_add(const Fq2& a, const Fq2& b) { return {fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
OG_HD Fq2 f_sub(const Fq2& a, const Fq2& b) { return {fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
OG_HD Fq2 f_dbl(const Fq2& a) { return {fe_dbl(a.c0), fe_dbl(a.c1)}; }
OG_HD Fq2 f_neg(const Fq2& a) { return {fe_neg(a.c0), fe_neg(a.c1)}; }
// Schoolbook over the carry-free 64-bit columns with TWO reductions instead of Karatsuba's three reductions and five
// modular add/subs: c0 = a0 b0 + (8N - a1) b1, c1 = a0 b1 + a1 b0, each accumulated before one Montgomery
// reduction (field.hip.h).  A three-product Karatsuba in the columns (P3 - P1 + P2') saves 81 multiply-adds per
// product but needs three live column sets: measured on the G2 accumulation kernel it spills (scratch 172 -> 332 B
// per lane at 2 waves/SIMD) and runs 18 % slower, so the four-product form stays.
OG_HD Fq2 f_mul(const Fq2& a, const Fq2& b) {
  return {fe_mul_add(a.c0, b.c0, fe_neg_lazy(a.c1), b.c1), fe_mul_add(a.c0, b.c1, a.c1, b.c0)};
}
// re = a0^2 + (8N - a1) a1 (45 + 81 products, one reduction), im = (2 a0) a1; operands may be weak (a0 < 8N, a1 < 8N - 2^232:
// fe_neg_lazy's bound; the group law squares P < 6N)
OG_HD Fq2 f_sqr(const Fq2& a) {
  return {fe_sqr_add(a.c0, fe_neg_lazy(a.c1), a.c1), fe_mul(fe_dbl_lazy(a.c0), a.c1)};
}
// a b - c d with one reduction per component
OG_HD Fq f_mul_sub(const Fq& a, const Fq& b, const Fq& c, const Fq& d) {
  return fe_mul_add(a, b, fe_neg_lazy(c), d);
}
OG_HD Fq2 f_mul_sub(const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) {
  const Fq na1 = fe_neg_lazy(a.c1), nc0 = fe_neg_lazy(c.c0), nc1 = fe_neg_lazy(c.c1);
  // re: a0 b0 - a1 b1 - c0 d0 + c1 d1     im: a0 b1 + a1 b0 - c0 d1 - c1 d0
  return {fe_mul_add4(a.c0, b.c0, na1, b.c1, nc0, d.c0, c.c1, d.c1), fe_mul_add4(a.c0, b.c1, a.c1, b.c0, nc0, d.c1, nc1, d.c0)};
}
OG_HD Fq2 f_inv(const Fq2& a) {
  Fq n = fe_add(fe_sqr(a.c0), fe_sqr(a.c1));
  Fq ni = fe_inv(n);
  return {fe_mul(a.c0, ni), fe_neg(fe_mul(a.c1, ni))};
}

// weak forms (field.hip.h): normalized limbs, value bounded by a small multiple of N, never stored
OG_HD Fq f_sub_weak(const Fq& a, const Fq& b) { return fe_sub_weak(a, b); }
OG_HD Fq f_add2_weak(const Fq& a, const Fq& b) { return fe_add2_weak(a, b); }
OG_HD bool f_weak_diff_is_zero(const Fq& d) { return fe_weak_diff_is_zero(d); }
OG_HD Fq2 f_sub_weak(const Fq2& a, const Fq2& b) { return {fe_sub_weak(a.c0, b.c0), fe_sub_weak(a.c1, b.c1)}; }
OG_HD Fq2 f_add2_weak(const Fq2& a, const Fq2& b) { return {fe_add2_weak(a.c0, b.c0), fe_add2_weak(a.c1, b.c1)}; }
OG_HD bool f_weak_diff_is_zero(const Fq2& d) { return fe_weak_diff_is_zero(d.c0) && fe_weak_diff_is_zero(d.c1); }
// a b - x + 4N with ONE reduction and no carry pass (field.hip.h fe_mul_plus): for x < 2N the result lies in (2N, 6N) and is
// limb-for-limb what f_sub_weak(f_mul(a, b), x) gives.  In Fq2 the lazily negated operand is a's (a.c1).
OG_HD Fq f_mul_minus(const Fq& a, const Fq& b, const Fq& x) { return fe_mul_plus(a, b, fe_neg_lazy4(x)); }
OG_HD Fq2 f_mul_minus(const Fq2& a, const Fq2& b, const Fq2& x) {
  return {fe_mul_add_plus(a.c0, b.c0, fe_neg_lazy(a.c1), b.c1, fe_neg_lazy4(x.c0)), fe_mul_add_plus(a.c0, b.c1, a.c1, b.c0, fe_neg_lazy4(x.c1))};
}
// (neg ? -y : y) z - x + 4N, one reduction per component: the sign of a signed-digit entry is applied to the OPERANDS of the
// product (4N - y limb-wise, no carries), never to y itself.  In Fq2, c0 = y0 z0 - y1 z1 flips to (4N - y0) z0 + y1 z1.
OG_HD Fq f_mul_minus_y(const Fq& y, bool neg, const Fq& z, const Fq& x) {
  const Fq ny = fe_neg_lazy4(y);
  Fq a;
#pragma unroll
  for (int i = 0; i < 9; i++) a.l[i] = neg ? ny.l[i] : y.l[i];
  return fe_mul_plus(a, z, fe_neg_lazy4(x));
}
OG_HD Fq2 f_mul_minus_y(const Fq2& y, bool neg, const Fq2& z, const Fq2& x) {
  const Fq n0 = fe_neg_lazy4(y.c0), n1 = fe_neg_lazy4(y.c1), m1 = fe_neg_lazy(y.c1);
  Fq a0, a1, s1;  // a0 = +-y0, a1 = +-y1, s1 = -+y1 (the operand of the subtracted term of c0)
#pragma unroll
  for (int i = 0; i < 9; i++) {
    a0.l[i] = neg ? n0.l[i] : y.c0.l[i];
    a1.l[i] = neg ? n1.l[i] : y.c1.l[i];
    s1.l[i] = neg ? y.c1.l[i] : m1.l[i];
  }
  return {fe_mul_add_plus(a0, z.c0, s1, z.c1, fe_neg_lazy4(x.c0)), fe_mul_add_plus(a0, z.c1, a1, z.c0, fe_neg_lazy4(x.c1))};
}

// a a - c d with one reduction per component: X3 = R^2 - PP (P + 2 X1) as rounds 1-6 computed it.  The group law below takes
// X3 through f_sqr_rider now; this form stays for the raw-field hooks and the interpreter's op tables, which drive it alone.
// Bounds (multiples of N): a < 6, c < 2, d < 10.  Fq: 36 + 4 * 10 = 76 N^2.  Fq2: re 36 + 8*6 + 4*10 + 2*10 = 144,
// im 36 + 36 + 40 + 40 = 152, all < 169 (field.hip.h) -- which is why c is negated against 4N, not 8N.
OG_HD Fq f_sqr_sub(const Fq& a, const Fq& c, const Fq& d) { return fe_sqr_add(a, fe_neg_lazy4(c), d); }
OG_HD Fq2 f_sqr_sub(const Fq2& a, const Fq2& c, const Fq2& d) {
  // re: a0^2 - a1^2 - c0 d0 + c1 d1     im: 2 a0 a1 - c0 d1 - c1 d0
  const Fq na1 = fe_neg_lazy(a.c1), nc0 = fe_neg_lazy4(c.c0), nc1 = fe_neg_lazy4(c.c1);
  return {fe_sqr_add3(a.c0, na1, a.c1, nc0, d.c0, c.c1, d.c1), fe_mul_add3(fe_dbl_lazy(a.c0), a.c1, nc0, d.c1, nc1, d.c0)};
}

// ---- the weak X coordinate (xyzz_madd_signed_w / xyzz_add_w) ------------------------------------------------------------
// Inside a chain of additions the running X (each Fq2 component of it) has normalized limbs and a value below 5.5N instead of
// 2N; Y, ZZ and ZZZ stay below 2N.  The forms below are the ones that meet it.
// a b - x + 6N for a weak x (fe_neg_lazy6), one reduction: in (0.5N, 7.2N).  In Fq2 the lazily negated operand is a's (a.c1 < 2N).
OG_HD Fq f_mul_minus6(const Fq& a, const Fq& b, const Fq& x) { return fe_mul_plus(a, b, fe_neg_lazy6(x)); }
OG_HD Fq2 f_mul_minus6(const Fq2& a, const Fq2& b, const Fq2& x) {
  return {fe_mul_add_plus(a.c0, b.c0, fe_neg_lazy(a.c1), b.c1, fe_neg_lazy6(x.c0)), fe_mul_add_plus(a.c0, b.c1, a.c1, b.c0, fe_neg_lazy6(x.c1))};
}
// a b for a < 2N and a weak or wide b (< 7.2N): the lazily negated operand of the Fq2 product is a's, against 4N (not 8N), which
// keeps PP P and PP X1 near N: (2 + 4) 7.2 = 43 N^2
OG_HD Fq f_mul_n4(const Fq& a, const Fq& b) { return fe_mul(a, b); }
OG_HD Fq2 f_mul_n4(const Fq2& a, const Fq2& b) {
  return {fe_mul_add(a.c0, b.c0, fe_neg_lazy4(a.c1), b.c1), fe_mul_add(a.c0, b.c1, a.c1, b.c0)};
}
// X3 = r^2 - (ppp + 2q) + 4N with one reduction per component: the subtrahend rides in the high columns (fe_rider4, limbs
// < 2^31), so X3 is the reduced square plus at most 4N -- weak.  r < 6N: Fq 36 N^2; Fq2 re 36 + 8 * 6 = 84, im 2 * 36 = 72.
OG_HD Fq f_sqr_rider(const Fq& r, const Fq& ppp, const Fq& q) { return fe_sqr_plus(r, fe_rider4(ppp, q)); }
OG_HD Fq2 f_sqr_rider(const Fq2& r, const Fq2& ppp, const Fq2& q) {
  return {fe_sqr_add_plus(r.c0, fe_neg_lazy(r.c1), r.c1, fe_rider4(ppp.c0, q.c0)), fe_mul_plus(fe_dbl_lazy(r.c0), r.c1, fe_rider4(ppp.c1, q.c1))};
}
// D = q - x + 6N for a weak x, as the operand of R D.  Fq: limb-wise, no carry pass (limbs < 2^29 + 2^30; the columns of
// R D + (8N - Y1) PPP hold 9 (1.5 + 1) 2^59 + 9 2^58 < 2^64).  Fq2: R D - Y1 PPP is four products, two of them with a lazy
// operand already (15.75 x 2^60 of the 2^64), so there D pays one carry pass per component.
OG_HD Fq f_q_minus(const Fq& q, const Fq& x) { return fe_add_lazy(q, fe_neg_lazy6(x)); }
OG_HD Fq2 f_q_minus(const Fq2& q, const Fq2& x) {
  Fq2 r;
  normalize29u(r.c0.l, fe_add_lazy(q.c0, fe_neg_lazy6(x.c0)).l);
  normalize29u(r.c1.l, fe_add_lazy(q.c1, fe_neg_lazy6(x.c1)).l);
  return r;
}
// weak X -> [0, 2N): where a point is stored or handed to code that assumes the invariant of field.hip.h
OG_HD Fq f_norm_weak(const Fq& a) { return fe_norm_weak(a); }
OG_HD Fq2 f_norm_weak(const Fq2& a) { return {fe_norm_weak(a.c0), fe_norm_weak(a.c1)}; }

template <class T> struct FieldIO;
template <> struct FieldIO<Fq> {
  static constexpr int BYTES = 32;
  OG_HD static Fq load(const uint8_t* p) { return fe_load<FqParams>(p); }
  OG_HD static void store(uint8_t* p, const Fq& v) { fe_store(p, v); }
  OG_HD static Fq to_mont(const Fq& v) { return fe_to_mont(v); }
  OG_HD static Fq from_mont(const Fq& v) { return fe_from_mont(v); }
};
template <> struct FieldIO<Fq2> {
  static constexpr int BYTES = 64;
  OG_HD static Fq2 load(const uint8_t* p) { return {fe_load<FqParams>(p), fe_load<FqParams>(p + 32)}; }
  OG_HD static void store(uint8_t* p, const Fq2& v) { fe_store(p, v.c0); fe_store(p + 32, v.c1); }
  OG_HD static Fq2 to_mont(const Fq2& v) { return {fe_to_mont(v.c0), fe_to_mont(v.c1)}; }
  OG_HD static Fq2 from_mont(const Fq2& v) { return {fe_from_mont(v.c0), fe_from_mont(v.c1)}; }
};

// ---- points -------------------------------------------------------------------
template <class T>
struct Affine {
  T x, y;
  static constexpr int BYTES = 2 * FieldIO<T>::BYTES;
  OG_HD bool is_inf() const { return x.is_zero() && y.is_zero(); }
  OG_HD static Affine inf() { return {T::zero(), T::zero()}; }
  // raw load/store of the in-HBM (Montgomery) representation
  OG_HD static Affine load(const uint8_t* p) {
    return {FieldIO<T>::load(p), FieldIO<T>::load(p + FieldIO<T>::BYTES)};
  }
  OG_HD void store(uint8_t* p) const {
    FieldIO<T>::store(p, x);
    FieldIO<T>::store(p + FieldIO<T>::BYTES, y);
  }
};

template <class T>
struct XYZZ {
  T x, y, zz, zzz;
  static constexpr int BYTES = 4 * FieldIO<T>::BYTES;
  OG_HD bool is_inf() const { return zz.is_zero(); }
  OG_HD static XYZZ inf() { return {T::one(), T::one(), T::zero(), T::zero()}; }
  OG_HD static XYZZ from_affine(const Affine<T>& a) {
    if (a.is_inf()) return inf();
    return {a.x, a.y, T::one(), T::one()};
  }
  OG_HD static XYZZ load(const uint8_t* p) {
    constexpr int B = FieldIO<T>::BYTES;
    return {FieldIO<T>::load(p), FieldIO<T>::load(p + B), FieldIO<T>::load(p + 2 * B), FieldIO<T>::load(p + 3 * B)};
  }
  OG_HD void store(uint8_t* p) const {
    constexpr int B = FieldIO<T>::BYTES;
    FieldIO<T>::store(p, x);
    FieldIO<T>::store(p + B, y);
    FieldIO<T>::store(p + 2 * B, zz);
    FieldIO<T>::store(p + 3 * B, zzz);
  }
};

template <class T>
OG_HD Affine<T> affine_neg(const Affine<T>& p) {
  return {p.x, f_neg(p.y)};
}

// 2*P for affine P (mdbl-2008-s-1)
template <class T>
OG_HD XYZZ<T> xyzz_dbl_affine(const Affine<T>& p) {
  if (p.is_inf() || p.y.is_zero()) return XYZZ<T>::inf();
  T U = f_dbl(p.y);
  T V = f_sqr(U);
  T W = f_mul(U, V);
  T S = f_mul(p.x, V);
  T xx = f_sqr(p.x);
  T M = f_add(f_dbl(xx), xx);
  T X3 = f_sub(f_sqr(M), f_dbl(S));
  T Y3 = f_mul_sub(M, f_sub(S, X3), W, p.y);
  return {X3, Y3, V, W};
}

// 2*P (dbl-2008-s-1)
template <class T>
OG_HD XYZZ<T> xyzz_dbl(const XYZZ<T>& p) {
  if (p.is_inf() || p.y.is_zero()) return XYZZ<T>::inf();
  T U = f_dbl(p.y);
  T V = f_sqr(U);
  T W = f_mul(U, V);
  T S = f_mul(p.x, V);
  T xx = f_sqr(p.x);
  T M = f_add(f_dbl(xx), xx);
  T X3 = f_sub(f_sqr(M), f_dbl(S));
  T Y3 = f_mul_sub(M, f_sub(S, X3), W, p.y);
  return {X3, Y3, f_mul(V, p.zz), f_mul(W, p.zzz)};
}

// acc + (neg ? -q : q), q affine (madd-2008-s); complete: handles acc = inf, q = inf, q = +-acc.
// Q = X1 PP is multiplied out ONCE: X3 = R^2 - PPP - 2Q takes PPP + 2Q as an addend of its reduction (f_sqr_rider) and
// D = Q - X3 is limb-wise (f_q_minus), where rounds 1-6 had R R - PP (P + 2 X1) and a second X1 PP inside D.  The price is
// that X3 leaves its reduction with up to 4N on top: a.x may be WEAK (normalized limbs, < 5.5N per component) and so is the
// result's x; y, zz, zzz are < 2N as everywhere.  Callers run chains of these and normalise x once (xyzz_norm), where the
// point is stored; xyzz_madd_signed below is the form that keeps the 2N contract per call.
//   * P = U2 - X1, R = S2 - Y1 come straight out of the Montgomery reduction of the product they follow (the subtrahend
//     rides in the high columns) -- no separate subtraction, no carry pass;
//   * the sign of a signed-digit entry negates q.y lazily (4N - y limb-wise, a multiplication operand); only the two rare
//     branches that need y itself negate it properly;
//   * q = +-acc is seen on PP (< 2N: exactly 0 or N iff P = 0 mod N), not on P, which now spans seven multiples of N.
// Bounds (multiples of N, Fq | per Fq2 component; a product routine returns < 1 + sum / 169.28):
//   X1 < 5.5       P = [x2 ZZ1] + 6N - X1: (0.5, 7.03 | 7.12)      R = [+-y2 ZZZ1] + 4N - Y1: (2, 5.05 | 5.15)
//   PP: 49.4 | 50.7 + 8 * 7.12 = 107.7 N^2 -> < 1.30 | 1.64        PPP = PP P: 9.2 | (1.64 + 4) 7.12 = 40.2 -> < 1.06 | 1.24
//   Q = PP X1: 7.2 | (1.64 + 4) 5.5 = 31.1 -> < 1.05 | 1.19        PPP + 2Q < 3.16 | 3.62 < 4N - 2^234 (fe_rider4)
//   X3 < [R^2] + 4N: 36 | 84 -> < 5.22 | 5.50: the invariant closes   D = Q + 6N - X3 < 7.05 | 7.19
//   Y3 = R D - Y1 PPP: 6 * 7.05 + 8 * 1.06 = 51 | 6 * 7.19 + 8 * 7.19 + 8 * 1.24 + 2 * 1.24 = 113 -> < 2
// 8 product sets + 2 squarings with 9 reductions and no carry pass (Fq2: two, in D).
template <class T>
OG_HD XYZZ<T> xyzz_madd_signed_w(const XYZZ<T>& a, const Affine<T>& q, bool neg) {
  if (q.is_inf()) return a;
  if (a.is_inf()) return XYZZ<T>::from_affine(neg ? affine_neg(q) : q);
  T P = f_mul_minus6(q.x, a.zz, a.x);         // U2 - X1 + 6N
  T R = f_mul_minus_y(q.y, neg, a.zzz, a.y);  // S2 - Y1 + 4N: (2, 6)   (operands <= 8N x 2N: far below 169 N^2)
  T PP = f_sqr(P);
  if (PP.is_zero()) {
    if (f_weak_diff_is_zero(R)) return xyzz_dbl_affine(neg ? affine_neg(q) : q);
    return XYZZ<T>::inf();
  }
  T PPP = f_mul_n4(PP, P);
  T Q = f_mul_n4(PP, a.x);
  T X3 = f_sqr_rider(R, PPP, Q);              // R^2 - PPP - 2Q + 4N: weak
  T D = f_q_minus(Q, X3);                     // Q - X3 + 6N
  T Y3 = f_mul_sub(R, D, a.y, PPP);           // R D - Y1 PPP
  return {X3, Y3, f_mul(a.zz, PP), f_mul(a.zzz, PPP)};
}

// the point with its weak x brought below 2N: before a store, and before code that assumes the invariant of field.hip.h
template <class T>
OG_HD XYZZ<T> xyzz_norm(const XYZZ<T>& p) {
  return {f_norm_weak(p.x), p.y, p.zz, p.zzz};
}

// the same with every coordinate of the result < 2N (a.x may still be weak)
template <class T>
OG_HD XYZZ<T> xyzz_madd_signed(const XYZZ<T>& a, const Affine<T>& q, bool neg) {
  return xyzz_norm(xyzz_madd_signed_w(a, q, neg));
}

template <class T>
OG_HD XYZZ<T> xyzz_madd(const XYZZ<T>& a, const Affine<T>& q) {
  return xyzz_madd_signed(a, q, false);
}

// a + b (add-2008-s); complete.  Same structure as xyzz_madd_signed_w with U1 = X1 ZZ2 in the place of X1: a.x and b.x may
// be weak (they only meet products), the result's x is weak.  U1, S1 < 2, so P and R are the (2, 6) differences against 4N
// and every bound above holds with room (Fq2: PP 84 N^2 -> < 1.5, PPP (1.5 + 4) 6 = 33, Q (1.5 + 4) 2 = 11, X3 < 5.5).
template <class T>
OG_HD XYZZ<T> xyzz_add_w(const XYZZ<T>& a, const XYZZ<T>& b) {
  if (b.is_inf()) return a;
  if (a.is_inf()) return b;
  T U1 = f_mul(a.x, b.zz);
  T S1 = f_mul(a.y, b.zzz);
  T P = f_mul_minus(b.x, a.zz, U1);        // U2 - U1 + 4N: (2, 6)
  T R = f_mul_minus(b.y, a.zzz, S1);       // S2 - S1 + 4N: (2, 6)
  if (f_weak_diff_is_zero(P)) {
    if (f_weak_diff_is_zero(R)) return xyzz_dbl(a);
    return XYZZ<T>::inf();
  }
  T PP = f_sqr(P);
  T PPP = f_mul_n4(PP, P);
  T Q = f_mul_n4(PP, U1);
  T X3 = f_sqr_rider(R, PPP, Q);
  T D = f_q_minus(Q, X3);                  // Q - X3 + 6N
  T Y3 = f_mul_sub(R, D, S1, PPP);
  return {X3, Y3, f_mul(f_mul(a.zz, b.zz), PP), f_mul(f_mul(a.zzz, b.zzz), PPP)};
}

// the same with every coordinate of the result < 2N
template <class T>
OG_HD XYZZ<T> xyzz_add(const XYZZ<T>& a, const XYZZ<T>& b) {
  return xyzz_norm(xyzz_add_w(a, b));
}

template <class T>
OG_HD XYZZ<T> xyzz_neg(const XYZZ<T>& p) {
  return {p.x, f_neg(p.y), p.zz, p.zzz};
}

// x = X/ZZ, y = Y/ZZZ (one inversion: 1/ZZZ, then 1/ZZ = ZZZ^-1 ... via ZZ^3 = ZZZ^2)
template <class T>
OG_HD Affine<T> xyzz_to_affine(const XYZZ<T>& p) {
  if (p.is_inf()) return Affine<T>::inf();
  T izzz = f_inv(p.zzz);
  // 1/ZZ = ZZ^2 / ZZ^3 = ZZ^2 / ZZZ^2 = (ZZ * izzz)^2
  T t = f_mul(p.zz, izzz);
  T izz = f_sqr(t);
  return {f_mul(p.x, izz), f_mul(p.y, izzz)};
}

// NO OUT-OF-LINE DEVICE FUNCTIONS.  On ROCm 7.2 / gfx950 every kernel that CALLED a device function
// taking or returning XYZZ<Fq2> (by reference, by pointer or by value) hung, while kernels that inline
// the same group law run correctly (bisected on the GPU in round 1; reproducer in the git history of tools/dbg/).  The whole EC layer is
// therefore __forceinline__, and kernels keep code size in check by having ONE textual site per
// primitive (add / dbl / madd / to_affine) driven by a small rolled "op loop" -- see msm_impl.hip.h.

typedef Affine<Fq> G1Affine;
typedef Affine<Fq2> G2Affine;
typedef XYZZ<Fq> G1XYZZ;
typedef XYZZ<Fq2> G2XYZZ;

}  // namespace og
