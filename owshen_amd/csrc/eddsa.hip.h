// BabyJubJub in projective twisted-Edwards coordinates: what the EdDSA kernels share (eddsa.hip: verification; eddsa_keys.hip:
// decompression, key derivation, signing).  Curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr with a = 168700, d = 168696
// (/root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs:174-189); everything is Fr arithmetic on the 9 x 29-bit layer.
#pragma once
#include "field.hip.h"

namespace og {

struct EdPoint {
  Fr x, y, z;
};

__device__ __forceinline__ Fr ed_const(uint32_t v) { return fe_to_mont(fe_from_u32<FrParams>(v)); }

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

__device__ __forceinline__ bool ed_on_curve(const Fr& x, const Fr& y, const Fr& ca, const Fr& cd) {
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

}  // namespace og
