// og_vk_load, host half: everything that depends on the verifying key alone, computed with og_verify's own decoder, Miller loop
// and affine step (verify_tower.h).  The kernels are in verify_gpu.hip.  Not part of libowshen_verify.so.
#include "verify_tower.h"
#include "verify_vk.h"
#include "key_blob.h"

namespace og {
namespace {
// xi^((p-1)/6): the Frobenius coefficient of w (canonical c0 || c1); its square is G12 (verify_tower.h)
static const uint8_t G11[64] = {0x70, 0xe4, 0xc9, 0xdc, 0xda, 0x35, 0x0b, 0xd6, 0x76, 0x21, 0x2f, 0x29, 0x08, 0x1e, 0x52, 0x5c, 0x60, 0x8b, 0xe6, 0x76, 0xdd, 0x9f, 0xb9, 0xe8, 0xdf, 0xa7, 0x65, 0x28, 0x1c, 0xb7, 0x84, 0x12,
    0xac, 0x62, 0xf3, 0x80, 0x5f, 0xf0, 0x5c, 0xca, 0xe5, 0xc7, 0xee, 0x8e, 0x77, 0x92, 0x79, 0x74, 0x8e, 0x0b, 0x15, 0x12, 0xfe, 0x7c, 0x32, 0xa6, 0xe6, 0xe7, 0xfa, 0xb4, 0xf3, 0x96, 0x69, 0x24};

void put_fq2(std::vector<uint8_t>& v, size_t slot, const Fq2& a) { FieldIO<Fq2>::store(v.data() + 64 * slot, a); }

// one step of a key point's twist walk through step()'s own slope() / advance(): slope and intercept recorded
bool walk_step(G2A& t, const G2A& q, uint8_t* out) {
  Fq2 lam;
  if (!slope(t, q, lam)) return false;
  FieldIO<Fq2>::store(out, lam);
  FieldIO<Fq2>::store(out + 64, f_sub(f_mul(lam, t.x), t.y));
  advance(t, q, lam);
  return true;
}

bool walk_all(const G2A& q, uint8_t* out) {
  G2A t = q;
  size_t s = 0;
  for (int i = 63; i >= 0; i--) {
    if (!walk_step(t, t, out + 128 * s++)) return false;
    if ((ATE_LOOP_LO >> i) & 1)
      if (!walk_step(t, q, out + 128 * s++)) return false;
  }
  const G2A q1 = {f_mul(fq2_conj(q.x), fq2_from_bytes(G12)), f_mul(fq2_conj(q.y), fq2_from_bytes(G13))};
  const G2A q2 = {f_mul(q.x, fq2_from_bytes(G22)), f_neg(f_mul(q.y, fq2_from_bytes(G23)))};
  return walk_step(t, q1, out + 128 * s++) && walk_step(t, q2, out + 128 * s++) && s == VK_WALK_STEPS;
}
}  // namespace

bool f12_plain_is_one(const uint32_t limbs[108]) {
  Fq2 co[6];
  for (int k = 0; k < 6; k++)
    for (int j = 0; j < 9; j++) {
      co[k].c0.l[j] = limbs[(2 * k) * 9 + j];
      co[k].c1.l[j] = limbs[(2 * k + 1) * 9 + j];
    }
  const Fq12 f = {{co[0], co[2], co[4]}, {co[1], co[3], co[5]}};
  return f12_is_one(final_exponentiation(f));
}

int vk_precompute(const uint8_t* vk, size_t vk_len, VkHost& out) {
  // the same tests as verify_cpu: what makes og_verify answer "invalid key" makes og_vk_load answer it
  VkView v;
  OG_TRY(vk_view(vk, vk_len, "og_vk_load", &v));
  const uint64_t n_pub = v.n_pub;
  const uint8_t *alpha_b = v.alpha1, *beta_b = v.beta2, *gamma_b = v.gamma2, *delta_b = v.delta2, *ic_b = v.ic;
  G1A alpha, icp;
  G2A beta, gamma, delta;
  bool inf;
  OG_REQUIRE(g1_decode(alpha_b, alpha, inf) && !inf && g2_decode(beta_b, beta, inf) && !inf && g2_decode(gamma_b, gamma, inf) && !inf &&
                 g2_decode(delta_b, delta, inf) && !inf,
             "og_vk_load: verifying key holds an invalid point");
  out.n_pub = n_pub;
  out.ic.assign((n_pub + 1) * 64, 0);
  for (size_t i = 0; i <= n_pub; i++) {
    OG_REQUIRE(g1_decode(ic_b + 64 * i, icp, inf), "og_vk_load: verifying key holds an invalid IC point");
    if (inf) continue;  // stays (0, 0)
    FieldIO<Fq>::store(out.ic.data() + 64 * i, icp.x);
    FieldIO<Fq>::store(out.ic.data() + 64 * i + 32, icp.y);
  }
  Fq12 m;
  OG_REQUIRE(miller_loop(alpha, beta, m), "og_vk_load: degenerate (alpha, beta)");
  const Fq2 co[6] = {m.c0.c0, m.c1.c0, m.c0.c1, m.c1.c1, m.c0.c2, m.c1.c2};  // coefficient of w^k: w^2 = v
  out.ab.resize(108);
  for (int k = 0; k < 6; k++)
    for (int j = 0; j < 9; j++) {
      out.ab[(2 * k) * 9 + j] = co[k].c0.l[j];
      out.ab[(2 * k + 1) * 9 + j] = co[k].c1.l[j];
    }
  out.walk.assign(2 * VK_WALK_STEPS * 128, 0);
  OG_REQUIRE(walk_all(gamma, out.walk.data()) && walk_all(delta, out.walk.data() + VK_WALK_STEPS * 128), "og_vk_load: degenerate twist walk");
  // constants of the kernels
  out.consts.assign(VK_N_CONSTS * 64, 0);
  const Fq half = fe_inv(fq_from_u32(2));
  put_fq2(out.consts, VK_C_HALF, Fq2{half, Fq::zero()});
  put_fq2(out.consts, VK_C_BT, fq2_scale(f_inv(Fq2{fq_from_u32(9), Fq::one()}), fq_from_u32(3)));
  put_fq2(out.consts, VK_C_G12, fq2_from_bytes(G12));
  put_fq2(out.consts, VK_C_G13, fq2_from_bytes(G13));
  put_fq2(out.consts, VK_C_G22, fq2_from_bytes(G22));
  put_fq2(out.consts, VK_C_G23, fq2_from_bytes(G23));
  // Frobenius on the coefficient of w^i: conjugate (odd powers of p) and multiply by xi^(i (p^k - 1) / 6).  With g = xi^((p-1)/6):
  // k = 1: g^i;  k = 2: (g conj(g))^i = N(g)^i;  k = 3: (g N(g))^i
  const Fq2 g = fq2_from_bytes(G11), ng = f_mul(g, fq2_conj(g)), g3 = f_mul(g, ng);
  Fq2 a = Fq2::one(), b = Fq2::one(), c = Fq2::one();
  for (int i = 0; i < 6; i++) {
    put_fq2(out.consts, VK_C_FROB + i, a);
    put_fq2(out.consts, VK_C_FROB + 6 + i, b);
    put_fq2(out.consts, VK_C_FROB + 12 + i, c);
    a = f_mul(a, g);
    b = f_mul(b, ng);
    c = f_mul(c, g3);
  }
  return OG_OK;
}

}  // namespace og
