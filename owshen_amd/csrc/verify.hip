// og_verify: Groth16 verification on the CPU (the `burn_tx` seam:
// /root/reference/src/blockchain/tx/burn_tx.rs:11-32 is where a sequencer would gate the debit on it).
// No reference counterpart (the snapshot verifies an ECDSA signature: contracts/src/Owshen.sol:66-78).
// The check is the EIP-197 predicate  e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) == 1  with
// vk_x = IC_0 + sum x_i IC_i, evaluated with an optimal-ate Miller loop (affine line functions) over the
// tower Fq2 = Fq[u]/(u^2+1), Fq6 = Fq2[v]/(v^3-(9+u)), Fq12 = Fq6[w]/(w^2-v) and a plain square-and-multiply
// final exponentiation.  It reuses the SAME 9 x 29-bit field layer and group law as the kernels, compiled for
// the host (no GPU is touched: the verifier must work on a sequencer without one).
#include "verify_tower.h"
#include "verify_vk.h"
#include "key_blob.h"

namespace og {

// the verifying key's layout: key_blob.h
int verify_cpu(const uint8_t* vk, size_t vk_len, const uint8_t* pub, size_t n_pub, const uint8_t* proof, int* ok) {
  *ok = 0;
  VkView v;
  OG_TRY(vk_view(vk, vk_len, "og_verify", &v));
  OG_REQUIRE(v.n_pub == n_pub, "og_verify: number of public inputs does not match the verifying key");
  const uint8_t *alpha_b = v.alpha1, *beta_b = v.beta2, *gamma_b = v.gamma2, *delta_b = v.delta2, *ic_b = v.ic;
  G1A alpha, A, Cc, icp;
  G2A beta, gamma, delta, B;
  bool inf;
  OG_REQUIRE(g1_decode(alpha_b, alpha, inf) && !inf && g2_decode(beta_b, beta, inf) && !inf && g2_decode(gamma_b, gamma, inf) && !inf &&
                 g2_decode(delta_b, delta, inf) && !inf,
             "og_verify: verifying key holds an invalid point");
  // proof points: invalid encodings / off-curve / wrong subgroup / infinity => reject (ok = 0), not an error
  bool ia, ib, ic;
  if (!g1_decode(proof, A, ia) || !g2_decode(proof + 64, B, ib) || !g1_decode(proof + 192, Cc, ic)) return OG_OK;
  if (ia || ib || ic) return OG_OK;
  // vk_x = IC_0 + sum x_i IC_i   (public inputs must be canonical Fr elements)
  XYZZ<Fq> vkx = XYZZ<Fq>::inf();
  for (size_t i = 0; i <= n_pub; i++) {
    OG_REQUIRE(g1_decode(ic_b + 64 * i, icp, inf), "og_verify: verifying key holds an invalid IC point");
    // a public input >= r is a reject whatever its IC base is (checked BEFORE the infinity shortcut: an input whose base is
    // the point at infinity contributes nothing, but it still has to be a field element)
    const uint8_t* xb = i ? pub + 32 * (i - 1) : nullptr;
    if (xb && !limbs_lt_modulus(xb, FrParams::N)) return OG_OK;
    if (inf) continue;
    const Affine<Fq> p = {icp.x, icp.y};
    if (i == 0) {
      vkx = xyzz_madd(vkx, p);
      continue;
    }
    const Fr x = ld_any<FrParams>(xb);
    XYZZ<Fq> t = XYZZ<Fq>::inf();
    for (int w = 8; w >= 0; w--)
      for (int bit = 28; bit >= 0; bit--) {
        t = xyzz_dbl(t);
        if ((x.l[w] >> bit) & 1) t = xyzz_madd(t, p);
      }
    vkx = xyzz_add(vkx, t);
  }
  Fq12 f = f12_one(), m;
  const G1A negA = {A.x, fe_neg(A.y)};
  if (!miller_loop(negA, B, m)) return OG_OK;
  f = f12_mul(f, m);
  if (!miller_loop(alpha, beta, m)) return OG_OK;
  f = f12_mul(f, m);
  if (!vkx.is_inf()) {
    const Affine<Fq> v = xyzz_to_affine(vkx);
    if (!miller_loop({v.x, v.y}, gamma, m)) return OG_OK;
    f = f12_mul(f, m);
  }
  if (!miller_loop(Cc, delta, m)) return OG_OK;
  f = f12_mul(f, m);
  *ok = f12_is_one(final_exponentiation(f)) ? 1 : 0;
  return OG_OK;
}

}  // namespace og
