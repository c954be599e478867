// Stealth notes: a note sealed to a public key, and the wallet's scan over every memo the pool has published (include/owshen_gpu.h,
// "stealth notes"; the scheme is defined in tests/note_spec.py).  The reference has no counterpart: its BabyJubJub file
// (src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs) supplies the curve and `multiply` (:68-78), which fixes what
// s * P means for every point of the curve, torsion included.  One item per lane, Fr arithmetic on the 9 x 29-bit layer, the curve
// law of eddsa.hip.h, the permutation of mimc7.hip.h.
//
//   scan   S = sk * E with ONE scalar for all lanes.  The host recodes sk once into a width-4 NAF (note_recode: digits 0, +-1, +-3,
//          +-5, +-7, at most 255 of them, about one in five non-zero) and hands the digits over as a kernel argument: they sit in
//          scalar registers, every branch on a digit is wave-uniform, and no lane waits for another lane's bit.  That buys a
//          dedicated doubling (ed_dbl: dbl-2008-bbjlp, 4 squarings + 4 products against the unified law's 12 products) for every
//          digit and an addition from a per-lane table E, 3E, 5E, 7E for the non-zero ones; the table lives in registers (see
//          DESIGN.md, row "f-5 notes", for the resource table that decided it).
//   KDF    k = H(S.x, S.y); the five outputs H(k, j) share the absorption of k (kdf_absorb_k), so each costs one permutation: four
//          permutations to the tag, and only a lane whose tag matches computes the rest.
//   owned  the form a wallet can use (tests/owned_note_spec.py): the ordinary note's secrets derive from S, which the SENDER knows too,
//          so the payer could spend what they paid.  The owned note is bound to P = pk + t BASE with t = H(k, 7); only the payee knows
//          x = sk + t mod l, and the claim statement (witness.hip) spends on knowledge of x.  Both kernels share the fronts of the
//          ordinary pair (note_seal_front, note_scan_front) and draw from the same sponge on indices 6 .. 9.
//   view   the owned scan needs sk, so whoever scans can spend.  The view form (tests/view_note_spec.py) splits the address into
//          PV = v BASE and PS = sk BASE: S = e PV = v E, P = PS + t BASE, the sponge on indices 10 .. 13.  k_note_scan_view holds v and
//          the public PS and opens t | amount | token | c; k_note_unlock, in the wallet, makes x = sk + t mod l and checks H(x BASE) = c.
//   seal   E = e * BASE from the 64 x 16 window table of eddsa_keys.hip, S = e * pk by a plain ladder over the unified law (one
//          addition site, no divergence), sixteen permutations.
#include "ctx.h"
#include "primitives.h"
#include "msm.hip.h"
#include "mimc7.hip.h"
#include "eddsa.hip.h"

namespace og {

// ---- the recoded scalar ------------------------------------------------------------------------------------------------------------
// A kernel's FORM = the NAF width W (digits are odd and below 2^(W-1) in magnitude: the table holds 2^(W-2) odd multiples), plus
// NOTE_FORM_UNIFIED for the A/B that doubles by the unified law.  The launches use NOTE_NAF_W; hooks builds also carry W = 3 (a table
// of two, OG_NOTE_NAF_W=3) and the unified doubling (OG_NOTE_DBL_UNIFIED=1): tools/note_scan_bench.py times them against each other.
constexpr int NOTE_NAF_W = 4;
constexpr int NOTE_FORM_UNIFIED = 16;
constexpr int NOTE_DIGITS = 256;      // a scalar below 2^254 has at most 255 digits

struct NoteDigits {
  int8_t d[NOTE_DIGITS];  // d[i] has weight 2^i
  int32_t top;            // the index of the highest non-zero digit, -1 for the scalar 0
};

// the width-w NAF of the integer in `scalar` (32 bytes little-endian, any value below 2^255): sum d[i] 2^i = scalar, every non-zero
// digit odd and below 2^(w-1) in magnitude ([-7, 7] for w = 4), any two of them at least w places apart.  The working copy is wiped
// before returning.
static void note_recode(const uint8_t scalar[32], int w, NoteDigits& out) {
  volatile uint32_t k[9];
  for (int i = 0; i < 8; i++) k[i] = (uint32_t)scalar[4 * i] | (uint32_t)scalar[4 * i + 1] << 8 | (uint32_t)scalar[4 * i + 2] << 16 | (uint32_t)scalar[4 * i + 3] << 24;
  k[8] = 0;
  out.top = -1;
  for (int i = 0; i < NOTE_DIGITS; i++) {
    int d = 0;
    if (k[0] & 1u) {
      const int m = (int)(k[0] & ((1u << w) - 1));
      d = m >= (1 << (w - 1)) ? m - (1 << w) : m;
      // k -= d: clears the low W bits; a negative digit carries upwards
      if (d > 0) {
        k[0] -= (uint32_t)d;  // (no borrow: the low bits are exactly d)
      } else {
        uint64_t c = (uint64_t)(-d);
        for (int j = 0; j < 9 && c; j++) {
          c += k[j];
          k[j] = (uint32_t)c;
          c >>= 32;
        }
      }
      out.top = i;
    }
    out.d[i] = (int8_t)d;
    for (int j = 0; j < 8; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 31);
    k[8] >>= 1;
  }
  for (int j = 0; j < 9; j++) k[j] = 0;
}

static void note_wipe(NoteDigits& dg) {
  volatile int8_t* p = dg.d;
  for (int i = 0; i < NOTE_DIGITS; i++) p[i] = 0;
  *(volatile int32_t*)&dg.top = -1;
}

static bool host_canonical_fr(const uint8_t v[32]) {  // the little-endian integer is below r
  uint32_t n[8];
  Fr m;
  for (int i = 0; i < 9; i++) m.l[i] = FrParams::N[i];
  fe_to_words(n, m);
  for (int i = 7; i >= 0; i--) {
    const uint32_t w = (uint32_t)v[4 * i] | (uint32_t)v[4 * i + 1] << 8 | (uint32_t)v[4 * i + 2] << 16 | (uint32_t)v[4 * i + 3] << 24;
    if (w != n[i]) return w < n[i];
  }
  return false;
}

// ---- the curve beside eddsa.hip.h ------------------------------------------------------------------------------------------------
// dedicated doubling (dbl-2008-bbjlp, the reference's projective double :152-164): 4 squarings, 3 products and the product by a.
// Like the unified law it has no exception on the curve: F = Z^2 (1 + d x^2 y^2) and J = -Z^2 (1 - d x^2 y^2) never vanish.
OG_HD EdPoint ed_dbl(const EdPoint& p, const Fr& ca) {
  const Fr B = fe_sqr(fe_add(p.x, p.y));
  const Fr C = fe_sqr(p.x);
  const Fr D = fe_sqr(p.y);
  const Fr E = fe_mul(ca, C);
  const Fr F = fe_add(E, D);
  const Fr J = fe_sub(F, fe_dbl(fe_sqr(p.z)));
  EdPoint r;
  r.x = fe_mul(fe_sub(fe_sub(B, C), D), J);
  r.y = fe_mul(F, fe_sub(E, D));
  r.z = fe_mul(F, J);
  return r;
}

// 8 P = (0, 1): P lies in the torsion subgroup of order 8 (P on the curve)
OG_HD bool ed_small(const Fr& x, const Fr& y, const Fr& ca) {
  EdPoint p;
  p.x = x;
  p.y = y;
  p.z = Fr::one();
#pragma unroll 1
  for (int k = 0; k < 3; k++) p = ed_dbl(p, ca);
  return p.x.is_zero() && p.y == p.z;
}

// s * (x, y) for the scalar recoded in `dg`, the same for every lane of the launch; (x, y) on the curve, Montgomery form; projective.
template <int FORM>
__device__ __forceinline__ EdPoint ed_mul_uniform(const NoteDigits& dg, const Fr& x, const Fr& y, const Fr& ca, const Fr& cd) {
  constexpr int NOTE_TAB = 1 << ((FORM & 15) - 2);
  constexpr bool UNIFIED = (FORM & NOTE_FORM_UNIFIED) != 0;
  EdPoint tab[NOTE_TAB];  // (2 k + 1) P: statically indexed everywhere, so it stays in registers
  tab[0].x = x;
  tab[0].y = y;
  tab[0].z = Fr::one();
  {
    const EdPoint p2 = ed_dbl(tab[0], ca);
#pragma unroll
    for (int k = 1; k < NOTE_TAB; k++) tab[k] = ed_add(tab[k - 1], p2, ca, cd);
  }
  EdPoint acc = ed_identity();
#pragma unroll 1
  for (int i = dg.top; i >= 0; i--) {
    acc = UNIFIED ? ed_add(acc, acc, ca, cd) : ed_dbl(acc, ca);
    const int d = dg.d[i];  // wave-uniform: a kernel argument
    if (d != 0) {
      const int idx = (d < 0 ? -d : d) >> 1;
      EdPoint q = tab[0];
#pragma unroll
      for (int k = 1; k < NOTE_TAB; k++) {
        if (idx == k) q = tab[k];
      }
      if (d < 0) q.x = fe_neg(q.x);  // -(x, y) = (-x, y)
      acc = ed_add(acc, q, ca, cd);
    }
  }
  return acc;
}

// ---- the KDF ---------------------------------------------------------------------------------------------------------------------
// one MultiMiMC7 absorption h <- h + x + E_h(x), E_h with its closing + h (mimc7.hip.h mimc7_hash2, one rolled round body)
__device__ __forceinline__ Fr note_absorb(const uint32_t* __restrict__ consts, const Fr& h, const Fr& x) {
  Fr t = x;
#pragma unroll 1
  for (int i = 0; i < MIMC7_ROUNDS; i++) {
    const Fr u = fe_add3_weak(t, h, mimc7_const(consts, i));
    const Fr u2 = fe_sqr(u);
    const Fr u4 = fe_sqr(u2);
    t = fe_mul(fe_mul(u4, u2), u);
  }
  return fe_add(fe_add(h, x), fe_add(t, h));
}

__device__ __forceinline__ Fr note_hash2(const uint32_t* __restrict__ consts, const Fr& l, const Fr& r) {
  return note_absorb(consts, note_absorb(consts, Fr::zero(), l), r);
}

// the sponge after k = H(S.x, S.y) has been absorbed: H(k, j) = note_absorb(consts, a, j) for every j
__device__ __forceinline__ Fr kdf_absorb_k(const uint32_t* __restrict__ consts, const Fr& sx, const Fr& sy) {
  return note_absorb(consts, Fr::zero(), note_hash2(consts, sx, sy));
}
enum { KDF_TAG = 1, KDF_NULLIFIER = 2, KDF_SECRET = 3, KDF_PAD_AMOUNT = 4, KDF_PAD_TOKEN = 5 };
// the owned form (tests/owned_note_spec.py) draws from the same sponge on indices of its own: neither scan sees the other form's tag
enum { KDF_OWNED_TAG = 6, KDF_OWNED_T = 7, KDF_OWNED_PAD_AMOUNT = 8, KDF_OWNED_PAD_TOKEN = 9 };
// and the view form (tests/view_note_spec.py) on a third set, in the owned form's order: tag, t, pad_a, pad_t
enum { KDF_VIEW_TAG = 10, KDF_VIEW_T = 11, KDF_VIEW_PAD_AMOUNT = 12, KDF_VIEW_PAD_TOKEN = 13 };

__device__ __forceinline__ bool fe_same_limbs(const Fr& a, const Fr& b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) x |= a.l[i] ^ b.l[i];
  return x == 0;
}

__device__ __forceinline__ bool below_2_128(const Fr& canonical) {
  uint32_t w[8];
  fe_to_words(w, canonical);
  return (w[4] | w[5] | w[6] | w[7]) == 0;
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------
// What both scans do with a memo before they know whose it is: the five fields canonical, E on the curve and not small, S = sk E,
// k = H(S.x, S.y) absorbed into `a`, and the tag H(k, tag_index) compared with the memo's.  true: the tag is this wallet's.
template <int FORM>
__device__ __forceinline__ bool note_scan_front(const uint32_t* __restrict__ consts, const NoteDigits& dg, const uint8_t* m, uint32_t tag_index, Fr& a) {
  bool good = true;
#pragma unroll 1
  for (int k = 0; k < 5; k++) good = good && canonical_fr(m + 32 * k);
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  {
    const Fr ex = fe_to_mont(fe_load<FrParams>(m)), ey = fe_to_mont(fe_load<FrParams>(m + 32));
    good = good && ed_on_curve(ex, ey, ca, cd) && !ed_small(ex, ey, ca);
    const EdPoint s = ed_mul_uniform<FORM>(dg, ex, ey, ca, cd);
    const Fr zi = fe_inv(s.z);  // never zero for a point of the curve; an off-curve E is refused whatever comes out
    a = kdf_absorb_k(consts, fe_mul(s.x, zi), fe_mul(s.y, zi));
  }
  const Fr tag = fe_from_mont(note_absorb(consts, a, ed_const(tag_index)));
  return good && fe_same_limbs(tag, fe_load<FrParams>(m + 64));
}

// memo: E.x | E.y | tag | amount + pad_a | token + pad_t.  hit 0: not this wallet's (or malformed); 1: opened -> nullifier' | secret' |
// amount | token; 2: the tag is this wallet's and the memo does not open (amount >= 2^128, or the leaf beside it is another).
template <int FORM>
__global__ void __launch_bounds__(64) k_note_scan(const uint32_t* __restrict__ consts, const NoteDigits dg, const uint8_t* __restrict__ memos,
                                                 const uint8_t* __restrict__ leaves, size_t n, uint8_t* __restrict__ opened, uint32_t* __restrict__ hit) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* m = memos + g * 160;
  Fr a;  // the sponge with k absorbed
  uint32_t code = note_scan_front<FORM>(consts, dg, m, KDF_TAG, a) ? 1u : 0u;
  uint8_t* o = opened ? opened + g * 128 : nullptr;
  if (code) {  // diverges; a wallet owns a vanishing share of the pool
    const Fr amount = fe_canon(fe_sub(fe_load<FrParams>(m + 96), fe_from_mont(note_absorb(consts, a, ed_const(KDF_PAD_AMOUNT)))));
    const Fr token = fe_canon(fe_sub(fe_load<FrParams>(m + 128), fe_from_mont(note_absorb(consts, a, ed_const(KDF_PAD_TOKEN)))));
    if (!below_2_128(amount)) code = 2u;
    if (code == 1u && (leaves || o)) {
      const Fr nul = note_absorb(consts, a, ed_const(KDF_NULLIFIER)), sec = note_absorb(consts, a, ed_const(KDF_SECRET));
      if (leaves) {
        const Fr leaf = note_hash2(consts, note_hash2(consts, nul, sec), note_hash2(consts, fe_to_mont(amount), fe_to_mont(token)));
        if (!fe_same_limbs(fe_from_mont(leaf), fe_load<FrParams>(leaves + g * 32))) code = 2u;
      }
      if (o && code == 1u) {
        fe_store(o, fe_from_mont(nul));
        fe_store(o + 32, fe_from_mont(sec));
        fe_store(o + 64, amount);
        fe_store(o + 96, token);
      }
    }
  }
  if (o && code != 1u) store_zeros(o, 8);
  hit[g] = code;
}

// ---- the owned form: a note bound to a one-time key P = pk + t BASE ----------------------------------------------------------------------
// sk mod l beside the recoded digits: a kernel argument like them, so it lives in scalar registers and nowhere else
struct NoteScalar {
  uint32_t w[8];
};

// k BASE, affine, for the integer in w (any value below 2^256): the 64 table additions of ed_mul_base and one inversion
__device__ __forceinline__ void note_mul_base_affine(const uint8_t* __restrict__ tab, const uint32_t w[8], const Fr& ca, const Fr& cd, Fr& x, Fr& y) {
  EdPoint p, unused;
  ed_mul_base<false>(tab, w, w, p, unused, ca, cd);
  const Fr zi = fe_inv(p.z);
  x = fe_mul(p.x, zi);
  y = fe_mul(p.y, zi);
}

// memo: E.x | E.y | tag | amount + pad_a | token + pad_t, the KDF on the owned indices.  hit 0 and 2 as k_note_scan; 1: opened ->
// x | amount | token | c with x = (sk + t) mod l and c = H(P.x, P.y), P = x BASE.  Only a lane whose tag matches computes t, x, P, c
// and the leaf.
template <int FORM>
__global__ void __launch_bounds__(64) k_note_scan_owned(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const NoteDigits dg,
                                                       const NoteScalar sk_mod_l, const uint8_t* __restrict__ memos, const uint8_t* __restrict__ leaves,
                                                       size_t n, uint8_t* __restrict__ opened, uint32_t* __restrict__ hit) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* m = memos + g * 160;
  Fr a;  // the sponge with k absorbed
  uint32_t code = note_scan_front<FORM>(consts, dg, m, KDF_OWNED_TAG, a) ? 1u : 0u;
  uint8_t* o = opened ? opened + g * 128 : nullptr;
  if (code) {  // diverges; a wallet owns a vanishing share of the pool
    const Fr amount = fe_canon(fe_sub(fe_load<FrParams>(m + 96), fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_PAD_AMOUNT)))));
    const Fr token = fe_canon(fe_sub(fe_load<FrParams>(m + 128), fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_PAD_TOKEN)))));
    if (!below_2_128(amount)) code = 2u;
    if (code == 1u && (leaves || o)) {
      // x = (sk + t) mod l on the integer words: t < r < 8 l, sk mod l < l
      uint32_t xw[8];
      fe_to_words(xw, fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_T))));
#pragma unroll 1
      for (int k = 0; k < 8; k++)
        if (!ed_below_order(xw)) ed_sub_order(xw);
      uint32_t carry = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {  // (below 2 l < 2^252: no carry out)
        const uint64_t v = (uint64_t)xw[k] + sk_mod_l.w[k] + carry;
        xw[k] = (uint32_t)v;
        carry = (uint32_t)(v >> 32);
      }
      if (!ed_below_order(xw)) ed_sub_order(xw);
      const Fr ca = ed_const(168700), cd = ed_const(168696);
      Fr px, py;
      note_mul_base_affine(tab, xw, ca, cd, px, py);
      const Fr c = note_hash2(consts, px, py);
      if (leaves) {
        const Fr leaf = note_hash2(consts, c, note_hash2(consts, fe_to_mont(amount), fe_to_mont(token)));
        if (!fe_same_limbs(fe_from_mont(leaf), fe_load<FrParams>(leaves + g * 32))) code = 2u;
      }
      if (o && code == 1u) {
        fe_store(o, fe_from_words<FrParams>(xw));
        fe_store(o + 32, amount);
        fe_store(o + 64, token);
        fe_store(o + 96, fe_from_mont(c));
      }
    }
  }
  if (o && code != 1u) store_zeros(o, 8);
  hit[g] = code;
}

// ---- the view form: find and open with the view scalar v, spend with sk ------------------------------------------------------------------
// The address is (PV, PS) = (v BASE, sk BASE); a note is sealed to S = e PV and bound to P = PS + t BASE.  The scan holds v and the
// PUBLIC point PS: it finds the memo, opens amount and token and computes P and c, and it never sees x = sk + t, which k_note_unlock
// computes in the wallet.
// PS as canonical words: a kernel argument, public, converted only by a lane that has a hit
struct NotePoint {
  uint32_t x[8], y[8];
};

// memo: E.x | E.y | tag | amount + pad_a | token + pad_t, the KDF on the view indices; the front is the owned scan's with another tag
// index.  hit 0 as k_note_scan; 2: the tag matches and the amount is >= 2^128, P = PS + t BASE is small, or the leaf beside the memo
// is another; 1: opened -> t | amount | token | c with t = H(k, 11) canonical and unreduced, c = H(P.x, P.y).
template <int FORM>
__global__ void __launch_bounds__(64) k_note_scan_view(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const NoteDigits dg,
                                                      const NotePoint ps, const uint8_t* __restrict__ memos, const uint8_t* __restrict__ leaves, size_t n,
                                                      uint8_t* __restrict__ opened, uint32_t* __restrict__ hit) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* m = memos + g * 160;
  Fr a;  // the sponge with k absorbed
  uint32_t code = note_scan_front<FORM>(consts, dg, m, KDF_VIEW_TAG, a) ? 1u : 0u;
  uint8_t* o = opened ? opened + g * 128 : nullptr;
  if (code) {  // diverges; a wallet owns a vanishing share of the pool
    const Fr amount = fe_canon(fe_sub(fe_load<FrParams>(m + 96), fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_PAD_AMOUNT)))));
    const Fr token = fe_canon(fe_sub(fe_load<FrParams>(m + 128), fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_PAD_TOKEN)))));
    if (!below_2_128(amount)) code = 2u;
    if (code == 1u) {
      const Fr t = fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_T)));
      const Fr ca = ed_const(168700), cd = ed_const(168696);
      Fr px, py;  // P = PS + t BASE, affine
      {
        uint32_t tw[8];
        fe_to_words(tw, t);
        EdPoint tb, q;
        {
          EdPoint unused;
          ed_mul_base<false>(tab, tw, tw, tb, unused, ca, cd);
        }
        q.x = fe_to_mont(fe_from_words<FrParams>(ps.x));
        q.y = fe_to_mont(fe_from_words<FrParams>(ps.y));
        q.z = Fr::one();
        const EdPoint p = ed_add(tb, q, ca, cd);
        const Fr zi = fe_inv(p.z);  // never zero: the host has checked that PS is on the curve
        px = fe_mul(p.x, zi);
        py = fe_mul(p.y, zi);
      }
      if (ed_small(px, py, ca)) code = 2u;
      const Fr c = note_hash2(consts, px, py);
      if (leaves && code == 1u) {
        const Fr leaf = note_hash2(consts, c, note_hash2(consts, fe_to_mont(amount), fe_to_mont(token)));
        if (!fe_same_limbs(fe_from_mont(leaf), fe_load<FrParams>(leaves + g * 32))) code = 2u;
      }
      if (o && code == 1u) {
        fe_store(o, t);
        fe_store(o + 32, amount);
        fe_store(o + 64, token);
        fe_store(o + 96, fe_from_mont(c));
      }
    }
  }
  if (o && code != 1u) store_zeros(o, 8);
  hit[g] = code;
}

// row: t | amount | token | c as k_note_scan_view opens it (or as anybody claims to have) -> x | amount | token | c with
// x = (sk + t) mod l, the opened row of k_note_scan_owned.  ok = 1: the four fields canonical, amount < 2^128, H(x BASE) = c and, when
// leaves are given, leaf = H(c, H(amount, token)); otherwise the row is zeroed.  Every lane does the same work up to the store.
__global__ void __launch_bounds__(64) k_note_unlock(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const NoteScalar sk_mod_l,
                                                   const uint8_t* __restrict__ rows, const uint8_t* __restrict__ leaves, size_t n, uint8_t* __restrict__ out,
                                                   uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* row = rows + g * 128;
  uint8_t* o = out + g * 128;
  bool good = true;
#pragma unroll 1
  for (int k = 0; k < 4; k++) good = good && canonical_fr(row + 32 * k);
  const Fr amount = fe_load<FrParams>(row + 32), token = fe_load<FrParams>(row + 64), c = fe_load<FrParams>(row + 96);
  good = good && below_2_128(amount);
  // x = (sk + t) mod l on the integer words: t < r < 8 l (a t that is not canonical is refused whatever comes out), sk mod l < l
  uint32_t xw[8];
  fe_to_words(xw, fe_load<FrParams>(row));
#pragma unroll 1
  for (int k = 0; k < 8; k++)
    if (!ed_below_order(xw)) ed_sub_order(xw);
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {  // (below 2 l < 2^252 for a canonical t: no carry out)
    const uint64_t v = (uint64_t)xw[k] + sk_mod_l.w[k] + carry;
    xw[k] = (uint32_t)v;
    carry = (uint32_t)(v >> 32);
  }
  if (!ed_below_order(xw)) ed_sub_order(xw);
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  Fr px, py;
  note_mul_base_affine(tab, xw, ca, cd, px, py);
  const Fr cx = fe_from_mont(note_hash2(consts, px, py));  // (computed by every lane, then compared: no lane skips a hash)
  good = fe_same_limbs(cx, c) && good;
  if (leaves) {  // (uniform)
    const Fr leaf = fe_from_mont(note_hash2(consts, fe_to_mont(c), note_hash2(consts, fe_to_mont(amount), fe_to_mont(token))));
    good = fe_same_limbs(leaf, fe_load<FrParams>(leaves + g * 32)) && good;
  }
  if (good) {
    fe_store(o, fe_from_words<FrParams>(xw));
    fe_store(o + 32, amount);
    fe_store(o + 64, token);
    fe_store(o + 96, c);
  } else {
    store_zeros(o, 8);
  }
  ok[g] = good ? 1u : 0u;
}

// ---- seal ------------------------------------------------------------------------------------------------------------------------
// What the seals do with a request of FIELDS fields before the KDF.  FIELDS = 5, e | pk.x | pk.y | amount | token: the ladder's point
// and the one-time key's base point are the same pk.  FIELDS = 7, e | PV.x | PV.y | PS.x | PS.y | amount | token (the view form): the
// ladder runs over PV, and PS, which the caller adds t BASE to, is checked here like PV.  All fields canonical, amount (field
// FIELDS - 2) < 2^128, the points on the curve and not small, E = e BASE from the window table (not the identity) and S = e pk (e PV)
// by the ladder, both brought to affine by one inversion.  false: the request is refused (the points are then meaningless).
template <int FIELDS>
__device__ __forceinline__ bool note_seal_front(const uint8_t* __restrict__ tab, const uint8_t* req, const Fr& ca, const Fr& cd, Fr& ex, Fr& ey, Fr& sx,
                                                Fr& sy) {
  static_assert(FIELDS == 5 || FIELDS == 7, "a seal request has five fields, or seven with a spend key of its own");
  bool good = true;
#pragma unroll 1
  for (int k = 0; k < FIELDS; k++) good = good && canonical_fr(req + 32 * k);
  good = good && below_2_128(fe_load<FrParams>(req + 32 * (FIELDS - 2)));
  if (FIELDS == 7) {
    const Fr qx = fe_to_mont(fe_load<FrParams>(req + 96)), qy = fe_to_mont(fe_load<FrParams>(req + 128));
    good = good && ed_on_curve(qx, qy, ca, cd) && !ed_small(qx, qy, ca);
  }
  uint32_t we[8];
  fe_to_words(we, fe_load<FrParams>(req));
  EdPoint ep, sp;
  {
    EdPoint unused;
    ed_mul_base<false>(tab, we, we, ep, unused, ca, cd);
  }
  good = good && !(ep.x.is_zero() && ep.y == ep.z);  // E = e BASE has odd order: small(E) is E = (0, 1), i.e. e = 0 (mod l)
  {
    const Fr px = fe_to_mont(fe_load<FrParams>(req + 32)), py = fe_to_mont(fe_load<FrParams>(req + 64));
    good = good && ed_on_curve(px, py, ca, cd) && !ed_small(px, py, ca);
    // S = e pk, most significant bit first over the 254-bit scalar.  One addition site: an even step doubles, an odd step adds pk or
    // the identity, so no lane diverges.
    sp = ed_identity();
#pragma unroll 1
    for (int step = 0; step < 2 * 254; step++) {
      const int bit = 253 - (step >> 1);
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) word = k == (bit >> 5) ? we[k] : word;
      const bool add = (step & 1) != 0, set = ((word >> (bit & 31)) & 1u) != 0;
      EdPoint q = sp;
      if (add) {
        q = ed_identity();
#pragma unroll
        for (int k = 0; k < 9; k++) {
          q.x.l[k] = set ? px.l[k] : q.x.l[k];
          q.y.l[k] = set ? py.l[k] : q.y.l[k];
        }
      }
      sp = ed_add(sp, q, ca, cd);
    }
  }
  // both points to affine by one inversion
  const Fr zi = fe_inv(fe_mul(ep.z, sp.z));
  const Fr ezi = fe_mul(zi, sp.z), szi = fe_mul(zi, ep.z);
  ex = fe_mul(ep.x, ezi);
  ey = fe_mul(ep.y, ezi);
  sx = fe_mul(sp.x, szi);
  sy = fe_mul(sp.y, szi);
  return good;
}

// request e | pk.x | pk.y | amount | token -> memo E.x | E.y | tag | amount + pad_a | token + pad_t and note c' | leaf
__global__ void __launch_bounds__(64) k_note_seal(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const uint8_t* __restrict__ reqs,
                                                 size_t n, uint8_t* __restrict__ memos, uint8_t* __restrict__ notes, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* req = reqs + g * 160;
  uint8_t* memo = memos + g * 160;
  uint8_t* note = notes + g * 64;
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  Fr ex, ey, sx, sy;
  const bool good = note_seal_front<5>(tab, req, ca, cd, ex, ey, sx, sy);
  const Fr a = kdf_absorb_k(consts, sx, sy);
  const Fr nul = note_absorb(consts, a, ed_const(KDF_NULLIFIER)), sec = note_absorb(consts, a, ed_const(KDF_SECRET));
  const Fr leaf = note_hash2(consts, note_hash2(consts, nul, sec),
                             note_hash2(consts, fe_to_mont(fe_load<FrParams>(req + 96)), fe_to_mont(fe_load<FrParams>(req + 128))));
  if (good) {
    fe_store(memo, fe_from_mont(ex));
    fe_store(memo + 32, fe_from_mont(ey));
    fe_store(memo + 64, fe_from_mont(note_absorb(consts, a, ed_const(KDF_TAG))));
    fe_store(memo + 96, fe_canon(fe_add(fe_load<FrParams>(req + 96), fe_from_mont(note_absorb(consts, a, ed_const(KDF_PAD_AMOUNT))))));
    fe_store(memo + 128, fe_canon(fe_add(fe_load<FrParams>(req + 128), fe_from_mont(note_absorb(consts, a, ed_const(KDF_PAD_TOKEN))))));
    fe_store(note, fe_from_mont(note_hash2(consts, nul, sec)));
    fe_store(note + 32, fe_from_mont(leaf));
  } else {
    store_zeros(memo, 10);
    store_zeros(note, 4);
  }
  ok[g] = good ? 1u : 0u;
}

// request e | pk.x | pk.y | amount | token -> memo E.x | E.y | tag | amount + pad_a | token + pad_t (the KDF on the owned indices) and
// note c | leaf with P = pk + t BASE, c = H(P.x, P.y), leaf = H(c, H(amount, token)).  Refused: what k_note_seal refuses, and small(P).
__global__ void __launch_bounds__(64) k_note_seal_owned(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab,
                                                       const uint8_t* __restrict__ reqs, size_t n, uint8_t* __restrict__ memos, uint8_t* __restrict__ notes,
                                                       uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* req = reqs + g * 160;
  uint8_t* memo = memos + g * 160;
  uint8_t* note = notes + g * 64;
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  Fr ex, ey, sx, sy;
  bool good = note_seal_front<5>(tab, req, ca, cd, ex, ey, sx, sy);
  const Fr a = kdf_absorb_k(consts, sx, sy);
  Fr px, py;  // P = pk + t BASE, affine
  {
    uint32_t tw[8];
    fe_to_words(tw, fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_T))));
    EdPoint tb, pk;
    {
      EdPoint unused;
      ed_mul_base<false>(tab, tw, tw, tb, unused, ca, cd);
    }
    pk.x = fe_to_mont(fe_load<FrParams>(req + 32));
    pk.y = fe_to_mont(fe_load<FrParams>(req + 64));
    pk.z = Fr::one();
    const EdPoint p = ed_add(tb, pk, ca, cd);
    const Fr zi = fe_inv(p.z);  // never zero for a pk of the curve; a pk off it is refused whatever comes out
    px = fe_mul(p.x, zi);
    py = fe_mul(p.y, zi);
    good = good && !ed_small(px, py, ca);
  }
  const Fr c = note_hash2(consts, px, py);
  const Fr leaf = note_hash2(consts, c, note_hash2(consts, fe_to_mont(fe_load<FrParams>(req + 96)), fe_to_mont(fe_load<FrParams>(req + 128))));
  if (good) {
    fe_store(memo, fe_from_mont(ex));
    fe_store(memo + 32, fe_from_mont(ey));
    fe_store(memo + 64, fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_TAG))));
    fe_store(memo + 96, fe_canon(fe_add(fe_load<FrParams>(req + 96), fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_PAD_AMOUNT))))));
    fe_store(memo + 128, fe_canon(fe_add(fe_load<FrParams>(req + 128), fe_from_mont(note_absorb(consts, a, ed_const(KDF_OWNED_PAD_TOKEN))))));
    fe_store(note, fe_from_mont(c));
    fe_store(note + 32, fe_from_mont(leaf));
  } else {
    store_zeros(memo, 10);
    store_zeros(note, 4);
  }
  ok[g] = good ? 1u : 0u;
}

// request e | PV.x | PV.y | PS.x | PS.y | amount | token -> memo E.x | E.y | tag | amount + pad_a | token + pad_t (the KDF on the view
// indices, S = e PV) and note c | leaf with P = PS + t BASE, c = H(P.x, P.y), leaf = H(c, H(amount, token)): k_note_seal_owned with the
// ladder's point and the one-time key's base point apart.  Refused: what note_seal_front<7> refuses, and small(P).
__global__ void __launch_bounds__(64) k_note_seal_view(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab,
                                                      const uint8_t* __restrict__ reqs, size_t n, uint8_t* __restrict__ memos, uint8_t* __restrict__ notes,
                                                      uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* req = reqs + g * 224;
  uint8_t* memo = memos + g * 160;
  uint8_t* note = notes + g * 64;
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  Fr ex, ey, sx, sy;
  bool good = note_seal_front<7>(tab, req, ca, cd, ex, ey, sx, sy);
  const Fr a = kdf_absorb_k(consts, sx, sy);
  Fr px, py;  // P = PS + t BASE, affine
  {
    uint32_t tw[8];
    fe_to_words(tw, fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_T))));
    EdPoint tb, ps;
    {
      EdPoint unused;
      ed_mul_base<false>(tab, tw, tw, tb, unused, ca, cd);
    }
    ps.x = fe_to_mont(fe_load<FrParams>(req + 96));
    ps.y = fe_to_mont(fe_load<FrParams>(req + 128));
    ps.z = Fr::one();
    const EdPoint p = ed_add(tb, ps, ca, cd);
    const Fr zi = fe_inv(p.z);  // never zero for a PS of the curve; a PS off it is refused whatever comes out
    px = fe_mul(p.x, zi);
    py = fe_mul(p.y, zi);
    good = good && !ed_small(px, py, ca);
  }
  const Fr c = note_hash2(consts, px, py);
  const Fr leaf = note_hash2(consts, c, note_hash2(consts, fe_to_mont(fe_load<FrParams>(req + 160)), fe_to_mont(fe_load<FrParams>(req + 192))));
  if (good) {
    fe_store(memo, fe_from_mont(ex));
    fe_store(memo + 32, fe_from_mont(ey));
    fe_store(memo + 64, fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_TAG))));
    fe_store(memo + 96, fe_canon(fe_add(fe_load<FrParams>(req + 160), fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_PAD_AMOUNT))))));
    fe_store(memo + 128, fe_canon(fe_add(fe_load<FrParams>(req + 192), fe_from_mont(note_absorb(consts, a, ed_const(KDF_VIEW_PAD_TOKEN))))));
    fe_store(note, fe_from_mont(c));
    fe_store(note + 32, fe_from_mont(leaf));
  } else {
    store_zeros(memo, 10);
    store_zeros(note, 4);
  }
  ok[g] = good ? 1u : 0u;
}

// ---- launches --------------------------------------------------------------------------------------------------------------------
int note_seal_owned(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  hipLaunchKernelGGL(k_note_seal_owned, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, requests_d, n, memos_d,
                     notes_d, ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// sk is reduced mod l here, once, and handed over beside its digits; both copies are wiped before returning, and the launch copies
// its arguments: neither sk nor anything derived from it stays in the context
int note_scan_owned(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d, uint32_t* hit_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  NoteDigits dg;
  NoteScalar sl;
  for (int i = 0; i < 8; i++) sl.w[i] = (uint32_t)sk[4 * i] | (uint32_t)sk[4 * i + 1] << 8 | (uint32_t)sk[4 * i + 2] << 16 | (uint32_t)sk[4 * i + 3] << 24;
  for (int k = 0; k < 8; k++)  // sk < r < 8 l
    if (!ed_below_order(sl.w)) ed_sub_order(sl.w);
  note_recode(sk, NOTE_NAF_W, dg);
  hipLaunchKernelGGL(k_note_scan_owned<NOTE_NAF_W>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, dg, sl,
                     memos_d, leaves_d, n, opened_d, hit_d);
  note_wipe(dg);
  {
    volatile uint32_t* p = sl.w;
    for (int i = 0; i < 8; i++) p[i] = 0;
  }
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int note_seal_view(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  hipLaunchKernelGGL(k_note_seal_view, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, requests_d, n, memos_d,
                     notes_d, ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

static void note_words(uint32_t w[8], const uint8_t v[32]) {
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)v[4 * i] | (uint32_t)v[4 * i + 1] << 8 | (uint32_t)v[4 * i + 2] << 16 | (uint32_t)v[4 * i + 3] << 24;
}

// PS is public and the same for every memo of a call: it is judged here, once, on the host, by the functions the kernels use
const char* note_ps_refusal(const uint8_t ps[64]) {
  if (!host_canonical_fr(ps) || !host_canonical_fr(ps + 32)) return "a coordinate of ps is not a canonical field element (>= r)";
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  const Fr x = fe_to_mont(fe_load<FrParams>(ps)), y = fe_to_mont(fe_load<FrParams>(ps + 32));
  if (!ed_on_curve(x, y, ca, cd)) return "ps is not on the curve";
  if (ed_small(x, y, ca)) return "ps is a small point (8 ps = (0, 1))";
  return nullptr;
}

// v is recoded like the sk of the other scans and wiped like it; PS goes over as words
int note_scan_view(og_ctx* ctx, const uint8_t v[32], const uint8_t ps[64], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d,
                   uint32_t* hit_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  NoteDigits dg;
  NotePoint pt;
  note_words(pt.x, ps);
  note_words(pt.y, ps + 32);
  note_recode(v, NOTE_NAF_W, dg);
  hipLaunchKernelGGL(k_note_scan_view<NOTE_NAF_W>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, dg, pt,
                     memos_d, leaves_d, n, opened_d, hit_d);
  note_wipe(dg);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// sk mod l is the launch's only secret: reduced here, handed over as a kernel argument, wiped before returning
int note_unlock(og_ctx* ctx, const uint8_t sk[32], const uint8_t* rows_d, const uint8_t* leaves_d, size_t n, uint8_t* unlocked_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  NoteScalar sl;
  note_words(sl.w, sk);
  for (int k = 0; k < 8; k++)  // sk < r < 8 l
    if (!ed_below_order(sl.w)) ed_sub_order(sl.w);
  hipLaunchKernelGGL(k_note_unlock, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, sl, rows_d, leaves_d, n,
                     unlocked_d, ok_d);
  {
    volatile uint32_t* p = sl.w;
    for (int i = 0; i < 8; i++) p[i] = 0;
  }
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int note_seal(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* memos_d, uint8_t* notes_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  hipLaunchKernelGGL(k_note_seal, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, requests_d, n, memos_d, notes_d,
                     ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

bool note_sk_canonical(const uint8_t sk[32]) { return host_canonical_fr(sk); }

int note_scan(og_ctx* ctx, const uint8_t sk[32], const uint8_t* memos_d, const uint8_t* leaves_d, size_t n, uint8_t* opened_d, uint32_t* hit_d) {
  if (n == 0) return OG_OK;
  NoteDigits dg;
  const uint32_t* consts = (const uint32_t*)ctx->mimc_consts_d;
  const dim3 grid(grid_for(n, 64)), block(64);
#ifdef OG_AB_HOOKS
  if (OG_HOOK_INT("OG_NOTE_DBL_UNIFIED", 0)) {
    note_recode(sk, NOTE_NAF_W, dg);
    hipLaunchKernelGGL(k_note_scan<NOTE_NAF_W + NOTE_FORM_UNIFIED>, grid, block, 0, ctx->stream, consts, dg, memos_d, leaves_d, n, opened_d, hit_d);
  } else if (OG_HOOK_INT("OG_NOTE_NAF_W", NOTE_NAF_W) == 3) {
    note_recode(sk, 3, dg);
    hipLaunchKernelGGL(k_note_scan<3>, grid, block, 0, ctx->stream, consts, dg, memos_d, leaves_d, n, opened_d, hit_d);
  } else
#endif
  {
    note_recode(sk, NOTE_NAF_W, dg);  // (the launch copies its arguments: nothing of sk outlives this function)
    hipLaunchKernelGGL(k_note_scan<NOTE_NAF_W>, grid, block, 0, ctx->stream, consts, dg, memos_d, leaves_d, n, opened_d, hit_d);
  }
  note_wipe(dg);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// ---- test seam (hooks builds only) -----------------------------------------------------------------------------------------------
#ifdef OG_AB_HOOKS
// the uniform-scalar multiplication alone: points x | y (canonical) -> s * P as x | y (canonical); ok = 0 and zeros for a
// non-canonical coordinate or a point off the curve
__global__ void __launch_bounds__(64) k_hook_ed_mul_uniform(const NoteDigits dg, const uint8_t* __restrict__ pts, size_t n, uint8_t* __restrict__ out,
                                                           uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  const Fr x = fe_to_mont(fe_load<FrParams>(pts + g * 64)), y = fe_to_mont(fe_load<FrParams>(pts + g * 64 + 32));
  const bool good = canonical_fr(pts + g * 64) && canonical_fr(pts + g * 64 + 32) && ed_on_curve(x, y, ca, cd);
  const EdPoint s = ed_mul_uniform<NOTE_NAF_W>(dg, x, y, ca, cd);
  const Fr zi = fe_inv(s.z);
  if (good) {
    fe_store(out + g * 64, fe_from_mont(fe_mul(s.x, zi)));
    fe_store(out + g * 64 + 32, fe_from_mont(fe_mul(s.y, zi)));
  } else {
    store_zeros(out + g * 64, 4);
  }
  ok[g] = good ? 1u : 0u;
}
#endif

}  // namespace og

#ifdef OG_AB_HOOKS
extern "C" int og_hook_ed_mul_uniform_d(og_ctx* ctx, const uint8_t scalar[32], const uint8_t* points_d, size_t n, uint8_t* out_d, uint32_t* ok_out) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && scalar && points_d && out_d && ok_out && n >= 1 && n <= ((size_t)1 << 24), "og_hook_ed_mul_uniform_d: bad argument");
    OG_REQUIRE(host_canonical_fr(scalar), "og_hook_ed_mul_uniform_d: the scalar is not below r");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    uint32_t* ok_d = nullptr;
    OG_TRY(arena_get(ctx, "eddsa.ok", n * 4, (void**)&ok_d));
    NoteDigits dg;
    note_recode(scalar, NOTE_NAF_W, dg);
    hipLaunchKernelGGL(k_hook_ed_mul_uniform, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, dg, points_d, n, out_d, ok_d);
    note_wipe(dg);
    OG_HIP(hipGetLastError());
    OG_HIP(hipMemcpyAsync(ok_out, ok_d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}
#endif
