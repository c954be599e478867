// The G1 group law in the wave-wide form: every XYZZ coordinate spread over nine lanes of a wave (field_w9.hip.h).
// Used by k_assemble_g1_muls_w9 (ecmul_impl.hip.h) and, in hooks builds, driven alone on raw limbs by og_hook_w9_ec_chain_d
// (field_ops.hip; tests/w9_ec_chain_cases.py holds the cases and the integer model of every line below).
//
// A product is ~90 instructions instead of 205, sums and differences are one instruction.  Strict products (29-bit digit: output
// < a b / 2^261 + N whatever the operands, a b < 169 N^2 asked for) keep the bounds closed without any extra reduction -- in
// multiples of N, coordinates between operations X < 9.3, Y < 5.7, ZZ, ZZZ < 1.2:
//   doubling (dbl-2008-s-1, 9 products):  U = 2Y < 11.4;  V = U^2 < 1.8;  W = U V < 1.2;  S = X V < 1.2;  M = 3 X^2 < 6.2;
//     X3 = M^2 - 2S + 8N < 9.3;  D = S - X3 + 16N < 17.2;  Y3 = M D - W Y + 4N < 5.7
//   addition (add-2008-s, 14 products):   U1, S1, U2, S2 < 1.2;  P = U2 - U1 + 4N, R = S2 - S1 + 4N < 5.2;  PP, PPP, Q, RR < 1.2;
//     X3 = RR - (PPP + 2Q) + 8N < 9.3;  D = Q - X3 + 16N < 17.2;  Y3 = R D - S1 PPP + 4N < 5.6
// Every difference adds K N in the borrow-free form (w9_kn_limb: K - 2 above the subtrahend's bound) and is carried before it is
// used again.  There is no branch for equal or opposite operands and none for infinity: the caller keeps them apart.
#pragma once
#include "field_w9.hip.h"

namespace og {

struct W9Pt {
  uint32_t x, y, zz, zzz;
};
__device__ __forceinline__ uint32_t w9q_mul(const U9& a, uint32_t b, uint32_t nj) { return w9_mul<FqParams, true, false>(a, b, nj); }
__device__ __forceinline__ W9Pt w9_xyzz_dbl(const W9Pt& p, uint32_t nj, int lane) {
  const uint32_t c4 = w9_kn_limb<FqParams, 4>(lane), c8 = w9_kn_limb<FqParams, 8>(lane), c16 = w9_kn_limb<FqParams, 16>(lane);
  const uint32_t U = 2u * p.y;
  const U9 Ua = w9_gather(U);
  const uint32_t V = w9q_mul(Ua, U, nj), W = w9q_mul(Ua, V, nj);
  const U9 Xa = w9_gather(p.x);
  const uint32_t S = w9q_mul(Xa, V, nj), M = 3u * w9q_mul(Xa, p.x, nj);
  const U9 Ma = w9_gather(M);
  const uint32_t X3 = w9_carry(w9_sub(w9q_mul(Ma, M, nj), w9_carry(2u * S, lane), c8), lane);
  const uint32_t D = w9_carry(w9_sub(S, X3, c16), lane);
  const U9 Wa = w9_gather(W);
  const uint32_t Y3 = w9_carry(w9_sub(w9q_mul(Ma, D, nj), w9q_mul(Wa, p.y, nj), c4), lane);
  return {X3, Y3, w9q_mul(w9_gather(V), p.zz, nj), w9q_mul(Wa, p.zzz, nj)};
}
__device__ __forceinline__ W9Pt w9_xyzz_add(const W9Pt& a, const W9Pt& b, uint32_t nj, int lane) {
  const uint32_t c4 = w9_kn_limb<FqParams, 4>(lane), c8 = w9_kn_limb<FqParams, 8>(lane), c16 = w9_kn_limb<FqParams, 16>(lane);
  const U9 zz2 = w9_gather(b.zz), zzz2 = w9_gather(b.zzz), zz1 = w9_gather(a.zz), zzz1 = w9_gather(a.zzz);
  const uint32_t U1 = w9q_mul(zz2, a.x, nj), S1 = w9q_mul(zzz2, a.y, nj);
  const uint32_t P = w9_carry(w9_sub(w9q_mul(zz1, b.x, nj), U1, c4), lane), R = w9_carry(w9_sub(w9q_mul(zzz1, b.y, nj), S1, c4), lane);
  const U9 Pa = w9_gather(P), Ra = w9_gather(R);
  const uint32_t PP = w9q_mul(Pa, P, nj);
  const U9 PPa = w9_gather(PP);
  const uint32_t PPP = w9q_mul(PPa, P, nj), Q = w9q_mul(PPa, U1, nj);
  const uint32_t X3 = w9_carry(w9_sub(w9q_mul(Ra, R, nj), w9_carry(PPP + 2u * Q, lane), c8), lane);
  const uint32_t D = w9_carry(w9_sub(Q, X3, c16), lane);
  const U9 PPPa = w9_gather(PPP);
  const uint32_t Y3 = w9_carry(w9_sub(w9q_mul(Ra, D, nj), w9q_mul(PPPa, S1, nj), c4), lane);
  return {X3, Y3, w9q_mul(PPa, w9q_mul(zz1, b.zz, nj), nj), w9q_mul(PPPa, w9q_mul(zzz1, b.zzz, nj), nj)};
}

}  // namespace og
