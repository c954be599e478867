// og_vk_load / og_verify_batch_d: batched Groth16 verification on the GPU (DESIGN.md "Batched verification").
// No reference counterpart (see verify.hip).  The decision, proof by proof, is og_verify's:
//   e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) == 1,   vk_x = IC_0 + sum x_i IC_i,
// one proof per lane, in three kernels that each get their own register budget:
//   k_vfy_prepare   canonical / on-curve / [r]B = inf / infinity / public-input range tests, vk_x from 4-bit fixed-base windows
//                   of the IC points (at most 64 mixed additions per public input), -A, B, vk_x, C written as a 320 B record
//   k_vfy_miller    ONE shared accumulator per proof: f <- f^2 l_B(-A) l_gamma(vk_x) l_delta(C) per doubling step and the same
//                   sharing at the addition steps (64 squarings where four serial loops do 256).  Only B's walk is live, in
//                   HOMOGENEOUS PROJECTIVE coordinates (Costello-Lange-Naehrig line coefficients: no inversion anywhere in the
//                   loop; the lines differ from the affine ones by Fq2 factors, which the final exponentiation's p^6 - 1 kills);
//                   gamma's and delta's slopes and intercepts come from the key's table.  f *= Miller(alpha, beta) at the end.
//   k_vfy_finalexp  easy part by conjugation, Frobenius and one Fq2 inversion; hard part by the Fuentes-Castaneda x-power chain
//                   with Granger-Scott cyclotomic squarings (see the kernel for the chain and why its extra factor is harmless).
//
// REGISTER PLAN.  An Fq12 is 108 limbs.  It is never held in registers as a whole: an Fq12 is addressed as six Fq2 coefficients
// of w^k (w^6 = xi = 9 + u) behind a (pointer, stride) view, limb-interleaved across the lanes of the wave (limb j of the lane
// at word j * stride + lane: conflict-free in LDS, coalesced in HBM), and every Fq12 routine is a ROLLED loop over coefficient
// indices around one Fq2 product site -- dynamic indexing is free in memory where it would force a register array to scratch.
// The Miller accumulator and its product target live in LDS (2 x 108 x 64 words = 54 KB per 64-lane block: two blocks per CU);
// the final exponentiation's eight Fq12 variables live in an HBM workspace (L2-resident: 3.4 KB per proof).  Registers hold
// B's walk (X, Y, Z: 54 limbs), the three line coefficients and the operands of one Fq2 product.
#include "ctx.h"
#include "ec.hip.h"
#include "msm.hip.h"
#include "verify_vk.h"
#include <string.h>

struct og_vk {
  uint64_t n_pub = 0;
  int device = 0;  // the ordinal, not the context: a handle may be freed after its context is gone
  uint8_t *consts_d = nullptr, *walk_d = nullptr, *ic_d = nullptr, *tab_d = nullptr;
  uint32_t* ab_d = nullptr;
  uint64_t tab_bytes = 0, dev_bytes = 0;
};

namespace og {

#define OG_DEV __device__ __forceinline__

constexpr int VFY_REC = 320;   // -A.x | -A.y | B.x | B.y | vk_x.x | vk_x.y | C.x | C.y  (Montgomery, 32 B per Fq)
constexpr int VFY_SLOTS = 8;   // Fq12 variables of the final exponentiation
constexpr uint64_t BN_X = 0x44e992b44a6909f1ull;      // the curve parameter x (63 bits)
constexpr uint64_t ATE_LO = 0x9d797039be763ba8ull;    // 6x + 2 below its leading one (verify.hip)

// ---- Fq12 behind a view -------------------------------------------------------------------------------------------------------
struct F12V {
  uint32_t* p;
  size_t s;
};
OG_DEV Fq2 v_ld(const F12V& a, int k) {
  Fq2 r;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    r.c0.l[j] = a.p[(size_t)(18 * k + j) * a.s];
    r.c1.l[j] = a.p[(size_t)(18 * k + 9 + j) * a.s];
  }
  return r;
}
OG_DEV void v_st(const F12V& a, int k, const Fq2& v) {
#pragma unroll
  for (int j = 0; j < 9; j++) {
    a.p[(size_t)(18 * k + j) * a.s] = v.c0.l[j];
    a.p[(size_t)(18 * k + 9 + j) * a.s] = v.c1.l[j];
  }
}
OG_DEV Fq2 d_scale(const Fq2& a, const Fq& k) { return {fe_mul(a.c0, k), fe_mul(a.c1, k)}; }
OG_DEV Fq2 d_conj(const Fq2& a) { return {a.c0, fe_neg(a.c1)}; }
OG_DEV Fq2 d_triple(const Fq2& a) { return f_add(f_dbl(a), a); }
// (a0 + a1 u)(9 + u) = 9 a0 - a1 + (a0 + 9 a1) u, 9 a = 8 a + a
OG_DEV Fq2 d_mul_xi(const Fq2& a) {
  const Fq2 n = f_add(f_dbl(f_dbl(f_dbl(a))), a);
  return {fe_sub(n.c0, a.c1), fe_add(a.c0, n.c1)};
}
OG_DEV Fq2 d_const(const uint8_t* consts, int slot) { return FieldIO<Fq2>::load(consts + 64 * slot); }

OG_DEV void v_copy(const F12V& o, const F12V& a) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) v_st(o, k, v_ld(a, k));
}
OG_DEV void v_set_one(const F12V& o) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) v_st(o, k, k == 0 ? Fq2::one() : Fq2::zero());
}
// o = a b (o distinct from a and b): schoolbook over w, the wrapped half times xi
OG_DEV void v_mul(const F12V& o, const F12V& a, const F12V& b) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      const bool wrap = i > k;
      const Fq2 pr = f_mul(v_ld(a, i), v_ld(b, wrap ? k - i + 6 : k - i));
      if (wrap) hi = f_add(hi, pr);
      else lo = f_add(lo, pr);
    }
    v_st(o, k, f_add(lo, d_mul_xi(hi)));
  }
}
// o = a^2 (o distinct from a): 21 products, the cross terms doubled
OG_DEV void v_sqr(const F12V& o, const F12V& a) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      const bool wrap = i > k;
      const int j = wrap ? k - i + 6 : k - i;
      if (i > j) continue;
      Fq2 pr = f_mul(v_ld(a, i), v_ld(a, j));
      if (i != j) pr = f_dbl(pr);
      if (wrap) hi = f_add(hi, pr);
      else lo = f_add(lo, pr);
    }
    v_st(o, k, f_add(lo, d_mul_xi(hi)));
  }
}
// o = a (l0 + l1 w + l3 w^3) (o distinct from a): a line has three non-zero coefficients
OG_DEV void v_mul_line(const F12V& o, const F12V& a, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fq2 acc = Fq2::zero();
#pragma unroll 1
    for (int t = 0; t < 3; t++) {
      const int d = t == 2 ? 3 : t;  // the power of w this term carries
      const bool wrap = d > k;
      Fq2 l;
#pragma unroll
      for (int j = 0; j < 9; j++) {
        l.c0.l[j] = t == 0 ? l0.c0.l[j] : t == 1 ? l1.c0.l[j] : l3.c0.l[j];
        l.c1.l[j] = t == 0 ? l0.c1.l[j] : t == 1 ? l1.c1.l[j] : l3.c1.l[j];
      }
      Fq2 pr = f_mul(v_ld(a, wrap ? k - d + 6 : k - d), l);
      if (wrap) pr = d_mul_xi(pr);
      acc = f_add(acc, pr);
    }
    v_st(o, k, acc);
  }
}
// Granger-Scott squaring of an element of the cyclotomic subgroup (o distinct from a).  Over Fq4 = Fq2[s], s = w^3, s^2 = xi,
// the pairs (a_m, a_(m+3)) are Fq4 elements: E_m = a_m^2 + xi a_(m+3)^2, X_m = 2 a_m a_(m+3), and
//   o_(2m) = 3 E_m - 2 a_(2m),   o_(2m+3) = 3 X_m + 2 a_(2m+3)   (index 2m + 3 = 7 wraps to 1 with a factor xi).
OG_DEV void v_cyc_sqr(const F12V& o, const F12V& a) {
#pragma unroll 1
  for (int m = 0; m < 3; m++) {
    const Fq2 lo = v_ld(a, m), hi = v_ld(a, m + 3);
    const Fq2 S = f_sqr(lo), H = f_sqr(hi);
    Fq2 X = f_sub(f_sub(f_sqr(f_add(lo, hi)), S), H);
    const Fq2 E = f_add(d_mul_xi(H), S);
    const int ke = 2 * m, kx = m == 2 ? 1 : 2 * m + 3;
    if (m == 2) X = d_mul_xi(X);
    v_st(o, ke, f_sub(d_triple(E), f_dbl(v_ld(a, ke))));
    v_st(o, kx, f_add(d_triple(X), f_dbl(v_ld(a, kx))));
  }
}
// o = a^(p^e), e = 1 | 2 | 3 (in place allowed): coefficient-wise conjugation (odd e) and the constant xi^(i (p^e - 1) / 6)
OG_DEV void v_frob(const F12V& o, const F12V& a, const uint8_t* consts, int e) {
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    Fq2 c = v_ld(a, i);
    if (e & 1) c = d_conj(c);
    v_st(o, i, f_mul(c, d_const(consts, VK_C_FROB + 6 * (e - 1) + i)));
  }
}
// a <- a^(p^6) in place: w -> -w
OG_DEV void v_conj(const F12V& a) {
#pragma unroll 1
  for (int i = 1; i < 6; i += 2) v_st(a, i, f_neg(v_ld(a, i)));
}
OG_DEV bool v_is_one(const F12V& a) {
  bool one = v_ld(a, 0) == Fq2::one();
#pragma unroll 1
  for (int i = 1; i < 6; i++) one = one && v_ld(a, i).is_zero();
  return one;
}

// ---- kernel 1: decode, checks, vk_x ---------------------------------------------------------------------------------------------
OG_DEV uint32_t fr_limb(int w) {  // limb w of r without indexing a private array
  uint32_t limb = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) limb = (k == w) ? FrParams::N[k] : limb;
  return limb;
}

__global__ void __launch_bounds__(64) k_vfy_prepare(const uint8_t* __restrict__ consts, const uint8_t* __restrict__ ic, const uint8_t* __restrict__ tab,
                                                   size_t n_pub, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ proofs, size_t n,
                                                   uint8_t* __restrict__ rec, uint32_t* __restrict__ state) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  state[g] = 0;  // reject unless everything below holds
  const uint8_t* pf = proofs + g * 256;
  bool good = true;
#pragma unroll 1
  for (int k = 0; k < 8; k++) good = good && fe_lt_modulus(fe_load<FqParams>(pf + 32 * k));
#pragma unroll 1
  for (size_t k = 0; k < n_pub; k++) good = good && fe_lt_modulus(fe_load<FrParams>(pub + (g * n_pub + k) * 32));
  if (!good) return;
  const Fq three = fe_to_mont(fe_from_u32<FqParams>(3));
  // A and C: on y^2 = x^3 + 3, not the point at infinity (0, 0)
  const Fq ax = fe_to_mont(fe_load<FqParams>(pf)), ay = fe_to_mont(fe_load<FqParams>(pf + 32));
  const Fq cx = fe_to_mont(fe_load<FqParams>(pf + 192)), cy = fe_to_mont(fe_load<FqParams>(pf + 224));
  good = good && !(ax.is_zero() && ay.is_zero()) && fe_sqr(ay) == fe_add(fe_mul(fe_sqr(ax), ax), three);
  good = good && !(cx.is_zero() && cy.is_zero()) && fe_sqr(cy) == fe_add(fe_mul(fe_sqr(cx), cx), three);
  // B: on the twist y^2 = x^3 + 3 / xi, not infinity, and in the r-torsion ([r]B = infinity, as og_verify tests it)
  const G2Affine B = {FieldIO<Fq2>::to_mont(FieldIO<Fq2>::load(pf + 64)), FieldIO<Fq2>::to_mont(FieldIO<Fq2>::load(pf + 128))};
  good = good && !B.is_inf() && f_sqr(B.y) == f_add(f_mul(f_sqr(B.x), B.x), d_const(consts, VK_C_BT));
  if (!good) return;
  {
    G2XYZZ acc = G2XYZZ::inf();
#pragma unroll 1
    for (int w = 8; w >= 0; w--) {
      const uint32_t limb = fr_limb(w);
#pragma unroll 1
      for (int bit = 28; bit >= 0; bit--) {
        acc = xyzz_dbl(acc);
        if ((limb >> bit) & 1) acc = xyzz_madd(acc, B);
      }
    }
    if (!acc.is_inf()) return;
  }
  // vk_x = IC_0 + sum x_i IC_i: table entry (i, j, d) = d 16^j IC_i, one mixed addition per non-zero nibble
  G1XYZZ vx = G1XYZZ::from_affine(G1Affine::load(ic));
#pragma unroll 1
  for (size_t i = 1; i <= n_pub; i++) {
    if (G1Affine::load(ic + 64 * i).is_inf()) continue;  // (the input's range was tested above, as og_verify does before this shortcut)
    const uint32_t* xw = reinterpret_cast<const uint32_t*>(pub + (g * n_pub + (i - 1)) * 32);
#pragma unroll 1
    for (int j = 0; j < 64; j++) {
      const uint32_t d = (xw[j >> 3] >> ((j & 7) * 4)) & 15u;
      if (d) vx = xyzz_madd(vx, G1Affine::load(tab + (((i - 1) * 64 + (size_t)j) * 15 + (d - 1)) * 64));
    }
  }
  uint32_t st = 1;
  uint8_t* r = rec + g * VFY_REC;
  if (!vx.is_inf()) {  // vk_x at infinity: its pairing is skipped
    st |= 2;
    const G1Affine v = xyzz_to_affine(vx);
    fe_store(r + 192, v.x);
    fe_store(r + 224, v.y);
  }
  fe_store(r, ax);
  fe_store(r + 32, fe_neg(ay));
  FieldIO<Fq2>::store(r + 64, B.x);
  FieldIO<Fq2>::store(r + 128, B.y);
  fe_store(r + 256, cx);
  fe_store(r + 288, cy);
  state[g] = st;
}

// ---- kernel 2: the shared Miller loop ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_vfy_miller(const uint8_t* __restrict__ consts, const uint8_t* __restrict__ walk, const uint32_t* ab,
                                                  const uint8_t* __restrict__ rec, const uint32_t* __restrict__ state, size_t n, uint32_t* ws) {
  OG_DYN_LDS(lds);
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint32_t st = state[g];
  if (!(st & 1)) return;
  uint32_t* L = reinterpret_cast<uint32_t*>(lds) + threadIdx.x;
  F12V f = {L, 64}, t = {L + 108 * 64, 64};
  v_set_one(f);
  const uint8_t* r = rec + g * VFY_REC;
  const Fq half = d_const(consts, VK_C_HALF).c0;
  Fq2 X = FieldIO<Fq2>::load(r + 64), Y = FieldIO<Fq2>::load(r + 128), Z = Fq2::one();
  int i = 63, tail = 0;
  bool pend_add = false;
#pragma unroll 1
  for (size_t s = 0; s < VK_WALK_STEPS; s++) {
    Fq2 c0, c1, c2;  // B's line: (c0 y_P) + (c1 x_P) w + c2 w^3
    if (i >= 0 && !pend_add) {
      v_sqr(t, f);
      { const F12V x = f; f = t; t = x; }
      // T <- 2T, tangent (Costello-Lange-Naehrig, homogeneous projective, b' = 3 / xi)
      const Fq2 a = d_scale(f_mul(X, Y), half), b = f_sqr(Y), c = f_sqr(Z);
      const Fq2 e = f_mul(d_const(consts, VK_C_BT), d_triple(c)), f3 = d_triple(e);
      const Fq2 gg = d_scale(f_add(b, f3), half), h = f_sub(f_sqr(f_add(Y, Z)), f_add(b, c));
      const Fq2 j = f_sqr(X), e2 = f_sqr(e);
      X = f_mul(a, f_sub(b, f3));
      Y = f_sub(f_sqr(gg), d_triple(e2));
      Z = f_mul(b, h);
      c0 = f_neg(h);
      c1 = d_triple(j);
      c2 = f_sub(e, b);
      pend_add = (ATE_LO >> i) & 1;
      i--;
    } else {
      // T <- T + Q with Q = B, then pi(B), then -pi^2(B)
      Fq2 xq = FieldIO<Fq2>::load(r + 64), yq = FieldIO<Fq2>::load(r + 128);
      if (!pend_add) {
        if (tail == 0) {
          xq = f_mul(d_conj(xq), d_const(consts, VK_C_G12));
          yq = f_mul(d_conj(yq), d_const(consts, VK_C_G13));
        } else {
          xq = f_mul(xq, d_const(consts, VK_C_G22));
          yq = f_neg(f_mul(yq, d_const(consts, VK_C_G23)));
        }
        tail++;
      }
      pend_add = false;
      const Fq2 theta = f_sub(Y, f_mul(yq, Z)), lambda = f_sub(X, f_mul(xq, Z));
      const Fq2 c = f_sqr(theta), d = f_sqr(lambda), e = f_mul(lambda, d), ff = f_mul(Z, c), gg = f_mul(X, d);
      const Fq2 h = f_sub(f_add(e, ff), f_dbl(gg));
      X = f_mul(lambda, h);
      Y = f_sub(f_mul(theta, f_sub(gg, h)), f_mul(e, Y));
      Z = f_mul(Z, e);
      c0 = lambda;
      c1 = f_neg(theta);
      c2 = f_sub(f_mul(theta, xq), f_mul(lambda, yq));
    }
    // f <- f l_B(-A) l_gamma(vk_x) l_delta(C): gamma's and delta's lines are  y_P - lambda x_P w + (lambda x_T - y_T) w^3  from the table
#pragma unroll 1
    for (int which = 0; which < 3; which++) {
      if (which == 1 && !(st & 2)) continue;
      if (which) {
        const uint8_t* e = walk + ((size_t)(which - 1) * VK_WALK_STEPS + s) * 128;
        c0 = Fq2::one();
        c1 = f_neg(FieldIO<Fq2>::load(e));
        c2 = FieldIO<Fq2>::load(e + 64);
      }
      const uint8_t* pp = r + (which == 0 ? 0 : which == 1 ? 192 : 256);
      const Fq xp = fe_load<FqParams>(pp), yp = fe_load<FqParams>(pp + 32);
      v_mul_line(t, f, d_scale(c0, yp), d_scale(c1, xp), c2);
      { const F12V x = f; f = t; t = x; }
    }
  }
  const F12V abv = {const_cast<uint32_t*>(ab), 1};
  v_mul(t, f, abv);
  const F12V out = {ws + g, n};
  v_copy(out, t);
}

// ---- kernel 3: the final exponentiation ---------------------------------------------------------------------------------------------
// out = conj(in^x): x-power by square-and-multiply, MSB first, cyclotomic squarings; `in` must lie in the cyclotomic subgroup.
// tmp is scratch; out, in, tmp distinct.
OG_DEV void v_exp_neg_x(F12V out, const F12V& in, F12V tmp) {
  const F12V out0 = out;
  v_copy(out, in);
#pragma unroll 1
  for (int b = 61; b >= 0; b--) {  // bit 62 is the leading one
    v_cyc_sqr(tmp, out);
    if ((BN_X >> b) & 1) {
      v_mul(out, tmp, in);
    } else {
      const F12V x = out; out = tmp; tmp = x;
    }
  }
  if (out.p != out0.p) v_copy(out0, out);
  v_conj(out0);
}

// EASY PART  f^((p^6 - 1)(p^2 + 1)).  The inverse comes from norms, not from a tower inversion: with c = f^(p^6) (w -> -w),
// N = f c lies in Fq6 (even powers of w only), and with u = N^(p^2), v = N^(p^4), n = N u v lies in Fq2, so
// f^-1 = c u v / n  and  f^(p^6 - 1) = c^2 u v / n: four Fq12 products, two Frobenius maps, one Fq2 inversion.
// HARD PART.  The Fuentes-Castaneda / Knapp / Rodriguez-Henriquez chain ("Faster hashing to G2", SAC 2011), three x-powers:
// it raises to  m (p^4 - p^2 + 1) / r  with  m = 2 x (6 x^2 + 3 x + 1).  og_verify raises to (p^12 - 1) / r exactly; both
// results lie in the subgroup of r-th roots of unity, one is the m-th power of the other, and
//   gcd(m, r) = 1:  r is PRIME (the group order), so it suffices that r divides none of 2, x, 6 x^2 + 3 x + 1 -- all three
//   are positive and smaller than r = 36 x^4 + 36 x^3 + 18 x^2 + 6 x + 1.
// Raising to a power prime to r permutes the r-th roots of unity and fixes 1 alone: "is one" is the same decision
// (tests/verify_batch_cases.py: case_final_exponentiation_pin runs this kernel and the plain power on the same Miller values of
// valid and of corrupted proofs; tests/test_verify_batch_abi.py checks the arithmetic of m on a transcription of the chain).
__global__ void __launch_bounds__(64) k_vfy_finalexp(const uint8_t* __restrict__ consts, const uint32_t* __restrict__ state, size_t n, uint32_t* ws,
                                                    uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  if (!(state[g] & 1)) {
    ok[g] = 0;
    return;
  }
  F12V S[VFY_SLOTS];
#pragma unroll
  for (int k = 0; k < VFY_SLOTS; k++) S[k] = {ws + (size_t)k * 108 * n + g, n};
  // easy part
  v_copy(S[1], S[0]);
  v_conj(S[1]);                    // c
  v_mul(S[2], S[0], S[1]);         // N
  v_frob(S[3], S[2], consts, 2);   // u
  v_frob(S[4], S[3], consts, 2);   // v
  v_mul(S[5], S[3], S[4]);         // u v
  v_mul(S[3], S[2], S[5]);         // n (in Fq2: coefficient 0)
  const Fq2 ninv = f_inv(v_ld(S[3], 0));
  v_sqr(S[2], S[1]);               // c^2
  v_mul(S[3], S[2], S[5]);         // c^2 u v
#pragma unroll 1
  for (int k = 0; k < 6; k++) v_st(S[3], k, f_mul(v_ld(S[3], k), ninv));  // f^(p^6 - 1)
  v_frob(S[4], S[3], consts, 2);
  v_mul(S[0], S[4], S[3]);         // R = f^((p^6 - 1)(p^2 + 1)): in the cyclotomic subgroup from here on (inverse = conjugate)
  // hard part
  v_exp_neg_x(S[1], S[0], S[7]);   // y0 = R^-x
  v_cyc_sqr(S[2], S[1]);           // y1 = y0^2
  v_cyc_sqr(S[3], S[2]);           // y2 = y1^2
  v_mul(S[4], S[3], S[2]);         // y3 = y2 y1
  v_exp_neg_x(S[3], S[4], S[7]);   // y4 = y3^-x
  v_cyc_sqr(S[5], S[3]);           // y5 = y4^2
  v_exp_neg_x(S[6], S[5], S[7]);   // y6 = y5^-x
  v_conj(S[4]);                    // y3 <- 1 / y3
  v_conj(S[6]);                    // y6 <- 1 / y6
  v_mul(S[5], S[6], S[3]);         // y7 = y6 y4
  v_mul(S[6], S[5], S[4]);         // y8 = y7 y3
  v_mul(S[4], S[6], S[2]);         // y9 = y8 y1
  v_mul(S[5], S[6], S[3]);         // y10 = y8 y4
  v_mul(S[3], S[5], S[0]);         // y11 = y10 R
  v_frob(S[5], S[4], consts, 1);   // y12 = y9^p
  v_mul(S[2], S[5], S[3]);         // y13 = y12 y11
  v_frob(S[5], S[6], consts, 2);   // y8^(p^2)
  v_mul(S[3], S[5], S[2]);         // y14
  v_conj(S[0]);                    // 1 / R
  v_mul(S[5], S[0], S[4]);         // y15 = y9 / R
  v_frob(S[2], S[5], consts, 3);   // y15^(p^3)
  v_mul(S[0], S[2], S[3]);         // the result
  ok[g] = v_is_one(S[0]) ? 1u : 0u;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
namespace {
int to_device(const void* src, size_t bytes, uint8_t** out, og_vk* vk) {
  OG_HIP(hipMalloc((void**)out, bytes ? bytes : 16));
  vk->dev_bytes += bytes;
  if (bytes) OG_HIP(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
  return OG_OK;
}

// (n_pub x 64 x 15) affine points d 16^j IC_i (Montgomery), built on the host with ONE inversion per IC point (Montgomery's trick)
void ic_windows(const VkHost& h, std::vector<uint8_t>& tab) {
  tab.assign(h.n_pub * 64 * 15 * 64, 0);
  std::vector<G1XYZZ> pts(64 * 15);
  std::vector<Fq> pre(64 * 15);
  for (size_t i = 1; i <= h.n_pub; i++) {
    const G1Affine p = G1Affine::load(h.ic.data() + 64 * i);
    if (p.is_inf()) continue;  // its rows are never read
    G1XYZZ base = G1XYZZ::from_affine(p);
    for (int j = 0; j < 64; j++) {
      G1XYZZ e = base;
      for (int d = 1; d <= 15; d++) {
        pts[j * 15 + d - 1] = e;
        e = xyzz_add(e, base);
      }
      base = e;  // 16 * base
    }
    Fq run = Fq::one();
    for (size_t k = 0; k < pts.size(); k++) {
      pre[k] = run;
      run = fe_mul(run, pts[k].zzz);
    }
    Fq inv = fe_inv(run);
    uint8_t* out = tab.data() + (i - 1) * 64 * 15 * 64;
    for (size_t k = pts.size(); k-- > 0;) {
      const Fq izzz = fe_mul(inv, pre[k]);
      inv = fe_mul(inv, pts[k].zzz);
      const Fq izz = fe_sqr(fe_mul(pts[k].zz, izzz));
      fe_store(out + 64 * k, fe_mul(pts[k].x, izz));
      fe_store(out + 64 * k + 32, fe_mul(pts[k].y, izzz));
    }
  }
}
}  // namespace

void vk_destroy(og_vk* vk) {
  if (!vk) return;
  (void)hipSetDevice(vk->device);
  for (void* p : {(void*)vk->consts_d, (void*)vk->walk_d, (void*)vk->ic_d, (void*)vk->tab_d, (void*)vk->ab_d})
    if (p) (void)hipFree(p);
  delete vk;
}

int vk_load(og_ctx* ctx, const uint8_t* blob, size_t len, og_vk** out) {
  VkHost h;
  OG_TRY(vk_precompute(blob, len, h));
  og_vk* vk = new og_vk();
  vk->device = ctx->device;
  vk->n_pub = h.n_pub;
  vk->tab_bytes = h.n_pub * 64 * 15 * 64;
  int rc = hipMalloc((void**)&vk->tab_d, vk->tab_bytes ? vk->tab_bytes : 16) == hipSuccess ? OG_OK : OG_ERR_HIP;  // the large one first
  if (rc != OG_OK) set_error("og_vk_load: no device memory for the IC window tables");
  if (rc == OG_OK) {
    try {  // (nothing may unwind past the handle: it owns device memory)
      std::vector<uint8_t> tab;
      ic_windows(h, tab);
      vk->dev_bytes += vk->tab_bytes;
      if (!tab.empty() && hipMemcpy(vk->tab_d, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("og_vk_load: table upload failed");
        rc = OG_ERR_HIP;
      }
    } catch (const std::exception& e) {
      set_error(std::string("og_vk_load: ") + e.what());
      rc = OG_ERR_INVALID;
    }
  }
  if (rc == OG_OK) rc = to_device(h.consts.data(), h.consts.size(), &vk->consts_d, vk);
  if (rc == OG_OK) rc = to_device(h.walk.data(), h.walk.size(), &vk->walk_d, vk);
  if (rc == OG_OK) rc = to_device(h.ic.data(), h.ic.size(), &vk->ic_d, vk);
  if (rc == OG_OK) rc = to_device(h.ab.data(), h.ab.size() * 4, (uint8_t**)&vk->ab_d, vk);
  if (rc != OG_OK) {
    vk_destroy(vk);
    return rc;
  }
  *out = vk;
  return OG_OK;
}

void vk_info(const og_vk* vk, uint64_t info[4]) {
  info[0] = vk->n_pub;
  info[1] = VK_WALK_STEPS;
  info[2] = vk->tab_bytes;
  info[3] = vk->dev_bytes;
}

// prepare + Miller for proofs [0, n) of a chunk; leaves state and workspace slot 0 (the Miller products) in the arena
static int verify_front(og_ctx* ctx, const og_vk* vk, const uint8_t* pub_d, const uint8_t* proofs_d, size_t n, uint32_t** state, uint32_t** ws) {
  uint8_t* rec = nullptr;
  OG_TRY(arena_get(ctx, "vfy.rec", n * VFY_REC, (void**)&rec));
  OG_TRY(arena_get(ctx, "vfy.state", n * 4, (void**)state));
  OG_TRY(arena_get(ctx, "vfy.ws", n * (size_t)VFY_SLOTS * 108 * 4, (void**)ws));
  const dim3 grid(grid_for(n, 64)), block(64);
  hipLaunchKernelGGL(k_vfy_prepare, grid, block, 0, ctx->stream, (const uint8_t*)vk->consts_d, (const uint8_t*)vk->ic_d, (const uint8_t*)vk->tab_d,
                     (size_t)vk->n_pub, pub_d, proofs_d, n, rec, *state);
  OG_HIP(hipGetLastError());
  OG_STEP(ctx, "vfy.prepare");
  hipLaunchKernelGGL(k_vfy_miller, grid, block, 2 * 108 * 64 * 4, ctx->stream, (const uint8_t*)vk->consts_d, (const uint8_t*)vk->walk_d,
                     (const uint32_t*)vk->ab_d, (const uint8_t*)rec, (const uint32_t*)*state, n, *ws);
  OG_HIP(hipGetLastError());
  OG_STEP(ctx, "vfy.miller");
  return OG_OK;
}

int verify_batch(og_ctx* ctx, const og_vk* vk, const uint8_t* pub_d, const uint8_t* proofs_d, size_t n, uint32_t* ok_out) {
  OG_REQUIRE(vk->device == ctx->device, "og_verify_batch_d: the key was loaded on another device");
  constexpr size_t CHUNK = 65536;  // bounds the workspace (3.4 KB per proof)
  for (size_t at = 0; at < n; at += CHUNK) {
    const size_t m = n - at < CHUNK ? n - at : CHUNK;
    uint32_t *state = nullptr, *ws = nullptr, *ok_d = nullptr;
    OG_TRY(arena_get(ctx, "vfy.ok", m * 4, (void**)&ok_d));
    OG_TRY(verify_front(ctx, vk, pub_d ? pub_d + at * vk->n_pub * 32 : nullptr, proofs_d + at * 256, m, &state, &ws));
    hipLaunchKernelGGL(k_vfy_finalexp, dim3(grid_for(m, 64)), dim3(64), 0, ctx->stream, (const uint8_t*)vk->consts_d, (const uint32_t*)state, m, ws, ok_d);
    OG_HIP(hipGetLastError());
    OG_STEP(ctx, "vfy.finalexp");
    OG_HIP(hipMemcpyAsync(ok_out + at, ok_d, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OG_OK;
}

}  // namespace og

#ifdef OG_AB_HOOKS
// Test seams of the hooks build (never in the shipped library, never in the header): the Miller products of a batch as opaque
// 432 B values, and the two final exponentiations -- the kernel's chain and og_verify's plain power -- on such values.
extern "C" int og_hook_verify_miller_d(og_ctx* ctx, const og_vk* vk, const uint8_t* pub_d, const uint8_t* proofs_d, size_t n, uint32_t* f_out,
                                       uint32_t* state_out) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && vk && proofs_d && f_out && state_out && n >= 1 && n <= 65536, "og_hook_verify_miller_d: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    uint32_t *state = nullptr, *ws = nullptr;
    OG_TRY(verify_front(ctx, vk, pub_d, proofs_d, n, &state, &ws));
    std::vector<uint32_t> raw(108 * n);
    OG_HIP(hipMemcpyAsync(raw.data(), ws, raw.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipMemcpyAsync(state_out, state, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t g = 0; g < n; g++)
      for (int k = 0; k < 108; k++) f_out[g * 108 + k] = raw[(size_t)k * n + g];
    return OG_OK;
  });
}

extern "C" int og_hook_final_exp_d(og_ctx* ctx, const og_vk* vk, const uint32_t* f_in, size_t n, uint32_t* ok_chain, uint32_t* ok_plain) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && vk && f_in && ok_chain && ok_plain && n >= 1 && n <= 65536, "og_hook_final_exp_d: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    uint32_t *state = nullptr, *ws = nullptr, *ok_d = nullptr;
    OG_TRY(arena_get(ctx, "vfy.state", n * 4, (void**)&state));
    OG_TRY(arena_get(ctx, "vfy.ws", n * (size_t)VFY_SLOTS * 108 * 4, (void**)&ws));
    OG_TRY(arena_get(ctx, "vfy.ok", n * 4, (void**)&ok_d));
    std::vector<uint32_t> raw(108 * n), ones(n, 1u);
    for (size_t g = 0; g < n; g++)
      for (int k = 0; k < 108; k++) raw[(size_t)k * n + g] = f_in[g * 108 + k];
    OG_HIP(hipMemcpyAsync(ws, raw.data(), raw.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(state, ones.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_vfy_finalexp, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint8_t*)vk->consts_d, (const uint32_t*)state, n, ws, ok_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipMemcpyAsync(ok_chain, ok_d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t g = 0; g < n; g++) ok_plain[g] = f12_plain_is_one(f_in + g * 108) ? 1u : 0u;
    return OG_OK;
  });
}
#endif
