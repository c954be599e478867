// BabyJubJub keys and signatures on the GPU: key decompression, key derivation and batched signing, the rest of the surface of
// /root/reference/src/blockchain/tx/owshen_airdrop/babyjubjub/mod.rs beside `verify` (eddsa.hip): `decompress` :88-98,
// `PrivateKey::to_pub` :207-209 and `PrivateKey::sign` :210-236 with the placeholder hash replaced by MultiMiMC7.  One item per
// lane, Fr arithmetic on the 9 x 29-bit layer, the curve law of eddsa.hip.h.
//
//   square root   y^2 v = u by Tonelli-Shanks for r - 1 = 2^28 q, non-residue 7, with the division folded into the one
//                 exponentiation and a FIXED trip count (fr_sqrt_ratio below)
//   k * BASE      64 additions from a table of the 64 x 16 affine points d 16^j BASE (k_ed_table, once per context), no doublings
//   s             (r + h sk) mod ORDER, ORDER = 8 l even: mod l on the Montgomery layer (FlParams), mod 8 from the low limbs,
//                 recombined by CRT (ed_sign_s)
//
// Compressed key: x canonical little-endian, the parity of the canonical y in bit 255, bit 254 clear (include/owshen_gpu.h).
#include "ctx.h"
#include "primitives.h"
#include "msm.hip.h"
#include "mimc7.hip.h"
#include "eddsa.hip.h"

namespace og {

// ---- square root -----------------------------------------------------------------------------------------------------------------
// r - 1 = 2^28 q, q odd.  FrSqrt::E = (q - 1) / 2 as 8 words (225 bits: the top word is 1); FrSqrt::Z = 7^q, a generator of the
// 2^28-th roots of unity (7 is a non-residue: the oracle's choice and the field's multiplicative generator, mod.rs:7-11).
struct FrSqrt {
  static constexpr uint32_t E[8] = {0x1f0fac9fu, 0xcdcb848au, 0x419f4243u, 0x0c0ac2e9u, 0xc2822db4u, 0x098d014du, 0x83227397u, 0x00000001u};
  static constexpr uint32_t Z[8] = {0x60c37c9cu, 0xd34f1ed9u, 0xd39329c8u, 0x3215cf6du, 0x3dd31f74u, 0x98865ea9u, 0x166d18b7u, 0x03ddb9f5u};
};

// y with y^2 v = u, for v != 0 (Montgomery form in and out); false when u / v has no square root (y is then meaningless).
// With w = u / v and e = (q - 1) / 2, Tonelli-Shanks starts from w^(e+1) and w^q.  No inversion: v^(r-1) = 1 gives
//   g = u v^(2^29 - 1) = w v^(2^29),   g^q = w^q  (v^(2^29 q) = v^(2 (r-1)) = 1),   w^(e+1) = u g^e v^(2^28 - 1),
// so one 225-bit exponentiation of g and 28 squarings of v replace an inversion plus an exponentiation.  The loop that follows
// is the fixed-trip form (RFC 9380 I.4): level i = 28 .. 2 squares t (i - 2) times and multiplies the correction in under a
// select, 351 squarings and 81 products whatever the input.  The data-dependent loop of the oracle would average about half of
// that per lane, but a wave pays its deepest lane, and with 64 lanes one of them is nearly always within a few levels of the
// worst case; its two inner trip counts would also diverge lane by lane.  Here every lane of every wave takes the same path.
// Either root may come out: the caller fixes the parity.  u = 0 gives y = 0, true.
__device__ __forceinline__ bool fr_sqrt_ratio(const Fr& u, const Fr& v, Fr& y) {
  Fr c = Fr::one(), pw = v;  // c = v^(2^k - 1), pw = v^(2^k)
#pragma unroll 1
  for (int k = 0; k < 28; k++) {
    c = fe_mul(c, pw);
    pw = fe_sqr(pw);
  }
  const Fr g = fe_mul(u, fe_mul(fe_sqr(c), v));
  Fr a = g;  // g^e, the exponent's top bit taken
#pragma unroll 1
  for (int w = 6; w >= 0; w--) {
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) word = k == w ? FrSqrt::E[k] : word;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      a = fe_sqr(a);
      if ((word >> b) & 1) a = fe_mul(a, g);  // wave-uniform: the exponent is a constant
    }
  }
  Fr r = fe_mul(fe_mul(u, a), c);  // w^(e+1)
  Fr t = fe_mul(g, fe_sqr(a));     // w^q: in the 2^28-th roots of unity, of order <= 2^27 iff w is a square
  uint32_t zw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) zw[k] = FrSqrt::Z[k];
  Fr z = fe_to_mont(fe_from_words<FrParams>(zw));
#pragma unroll 1
  for (int i = 28; i >= 2; i--) {
    Fr b = t;
#pragma unroll 1
    for (int j = 0; j < i - 2; j++) b = fe_sqr(b);
    const bool keep = b == Fr::one();  // t^(2^(i-2)) == 1: t's order is already below 2^(i-1)
    const Fr rz = fe_mul(r, z);
    z = fe_sqr(z);
    const Fr tz = fe_mul(t, z);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      r.l[k] = keep ? r.l[k] : rz.l[k];
      t.l[k] = keep ? t.l[k] : tz.l[k];
    }
  }
  y = r;
  return fe_mul(fe_sqr(r), v) == u;
}

// ---- compressed keys -------------------------------------------------------------------------------------------------------------
// decompress (mod.rs:88-98): y = sqrt((1 - a x^2) / (1 - d x^2)), negated when its parity differs from the flag.  1 - d x^2 is
// never zero (d is a non-residue).  x, y canonical (not Montgomery) out; false: the encoding is refused or there is no root.
__device__ __forceinline__ bool ed_decompress(const uint8_t* p, Fr& x, Fr& y) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w & 0x7fffffffu};
  const uint32_t odd = hi.w >> 31;
  x = fe_from_words<FrParams>(w);
  const bool encoded = fe_lt_modulus(x) && ((hi.w >> 30) & 1u) == 0;
  const Fr xx = fe_sqr(fe_to_mont(x));
  const Fr u = fe_sub(Fr::one(), fe_mul(ed_const(168700), xx)), v = fe_sub(Fr::one(), fe_mul(ed_const(168696), xx));
  Fr ym;
  const bool root = fr_sqrt_ratio(u, v, ym);
  y = fe_from_mont(ym);
  const Fr ny = fe_canon(fe_neg(y));  // r - y, and 0 for y = 0
  const bool as_flagged = (y.l[0] & 1u) == odd;
#pragma unroll
  for (int k = 0; k < 9; k++) y.l[k] = as_flagged ? y.l[k] : ny.l[k];
  return encoded && root;
}

// compress (mod.rs:82-84) of canonical x, y
__device__ __forceinline__ void ed_store_compressed(uint8_t* p, const Fr& x, const Fr& y) {
  uint32_t w[8];
  fe_to_words(w, x);
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7] | ((y.l[0] & 1u) << 31));
}

__global__ void __launch_bounds__(64) k_eddsa_decompress(const uint8_t* __restrict__ in, size_t in_stride, size_t n, uint8_t* __restrict__ out,
                                                        size_t out_stride, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* src = in + g * in_stride;
  uint8_t* dst = out + g * out_stride;
  Fr x, y;
  const bool good = ed_decompress(src, x, y);
  if (good) {
    fe_store(dst, x);
    fe_store(dst + 32, y);
  } else {
    store_zeros(dst, 4);
  }
  for (size_t k = 32; k < in_stride; k += 16)  // what follows the key in a record follows the point
    *reinterpret_cast<uint4*>(dst + 32 + k) = *reinterpret_cast<const uint4*>(src + k);
  ok[g] = good ? 1u : 0u;
}

// ---- k * BASE from the window table ------------------------------------------------------------------------------------------------
// tab[j][d] = d 16^j BASE, affine x | y in Montgomery form (d = 0: the identity (0, 1), so a zero digit is an addition like any
// other).  Lane j: 4 j doublings of BASE, then the sixteen multiples, each brought to affine by its own inversion -- one wave, once
// per context.  One addition site: steps below 4 j double p, the rest store acc and add p to it.
__global__ void __launch_bounds__(64) k_ed_table(uint8_t* __restrict__ tab) {
  const int j = threadIdx.x;
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  // BASE (mod.rs:177-188)
  const uint32_t BX[8] = {0xbb957051u, 0x2893f3f6u, 0x0534e0b6u, 0x2ab8d801u, 0x9d6277c1u, 0x4eacb2e0u, 0xd63e739bu, 0x0bb77a6au};
  const uint32_t BY[8] = {0x872d7d8bu, 0x4b3c257au, 0xb9e13377u, 0xfce0051fu, 0xd16bf9edu, 0x25572e1cu, 0xf7a0b249u, 0x25797203u};
  EdPoint p, acc;
  p.x = fe_to_mont(fe_from_words<FrParams>(BX));
  p.y = fe_to_mont(fe_from_words<FrParams>(BY));
  p.z = Fr::one();
  acc.x = Fr::zero();
  acc.y = Fr::one();
  acc.z = Fr::one();
#pragma unroll 1
  for (int step = 0; step < 4 * j + ED_TAB_DIGITS; step++) {
    const bool dbl = step < 4 * j;
    if (!dbl) {
      const Fr zi = fe_inv(acc.z);  // never zero: the law is complete on the curve
      uint8_t* e = tab + (size_t)(j * ED_TAB_DIGITS + (step - 4 * j)) * 64;
      fe_store(e, fe_mul(acc.x, zi));
      fe_store(e + 32, fe_mul(acc.y, zi));
    }
    const EdPoint sum = ed_add(dbl ? p : acc, p, ca, cd);
    if (dbl) p = sum;
    else acc = sum;
  }
}

__global__ void __launch_bounds__(64) k_eddsa_pubkey(const uint8_t* __restrict__ tab, const uint8_t* __restrict__ sks, size_t n, uint8_t* __restrict__ pk,
                                                    uint8_t* __restrict__ pkc, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const bool good = canonical_fr(sks + g * 32);
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  uint32_t w[8];
  fe_to_words(w, fe_load<FrParams>(sks + g * 32));
  EdPoint p, unused;
  ed_mul_base<false>(tab, w, w, p, unused, ca, cd);
  const Fr zi = fe_inv(p.z);
  const Fr x = fe_from_mont(fe_mul(p.x, zi)), y = fe_from_mont(fe_mul(p.y, zi));
  if (pk) {
    if (good) {
      fe_store(pk + g * 64, x);
      fe_store(pk + g * 64 + 32, y);
    } else {
      store_zeros(pk + g * 64, 4);
    }
  }
  if (pkc) {
    if (good) ed_store_compressed(pkc + g * 32, x, y);
    else store_zeros(pkc + g * 32, 2);
  }
  ok[g] = good ? 1u : 0u;
}

// ---- s = (r + h sk) mod ORDER -------------------------------------------------------------------------------------------------------
// ORDER = 8 l is even: no Montgomery modulus.  l (the prime order of BASE, 251 bits) is one: the same product routines with these
// parameters (R = 2^261 > 4 l) give the sum mod l; the sum mod 8 comes from the operands' low limbs; and as l = 1 (mod 8),
//   s = s_l + l ((s_8 - s_l) mod 8)   is the one value below 8 l with both residues.
struct FlParams {
  static constexpr uint32_t N[9] = {0x192126f1u, 0x1b94bee1u, 0x083b8299u, 0x1ddb7072u, 0x02b0bab3u, 0x045b6818u, 0x1014dc28u, 0x19cb84c6u, 0x00060c89u};
  static constexpr uint32_t N2[9] = {0x12424de2u, 0x17297dc3u, 0x10770533u, 0x1bb6e0e4u, 0x05617567u, 0x08b6d030u, 0x0029b850u, 0x1397098du, 0x000c1913u};
  static constexpr uint32_t ONE[9] = {0x16a80956u, 0x1f4669ceu, 0x153f3e36u, 0x155f43afu, 0x05448452u, 0x148b709eu, 0x11ab93b7u, 0x1193be1bu, 0x0001af22u};  // 2^261 mod l
  static constexpr uint32_t R2[9] = {0x1a277d5du, 0x0440c552u, 0x0eb25d5au, 0x12a91d12u, 0x0abdceefu, 0x12585826u, 0x035d6897u, 0x1f152bb7u, 0x00016b61u};   // 2^522 mod l
  static constexpr uint32_t INV = 0x1c48f5efu;  // -l^-1 mod 2^29
};
typedef Fe<FlParams> Fl;

__device__ __forceinline__ Fl fl_of(const Fr& a) {  // the same integer, read mod l
  Fl r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = a.l[k];
  return r;
}

// r, h, sk: canonical integers below the field modulus (< 8.0001 l: within fe_mul's operand bound for l).  The result's limbs hold
// the integer s < ORDER < 2^254; the caller compares it with the field modulus.
__device__ __forceinline__ Fr ed_sign_s(const Fr& r, const Fr& h, const Fr& sk) {
  const Fl hs = fe_mul(fl_of(h), fe_to_mont(fl_of(sk)));  // h sk mod l, out of Montgomery form again: (h)(sk R) / R
  const Fl rl = fe_mul(fl_of(r), Fl::one());              // r mod l likewise: (r)(R) / R
  const Fl sl = fe_canon(fe_add(hs, rl));
  const uint32_t s8 = (r.l[0] + h.l[0] * sk.l[0]) & 7u;
  const uint32_t k = (s8 - sl.l[0]) & 7u;
  Fr s;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    c += (uint64_t)sl.l[i] + (uint64_t)k * FlParams::N[i];
    s.l[i] = (uint32_t)c & MASK29;
    c >>= 29;
  }
  return s;
}

// ---- signing ---------------------------------------------------------------------------------------------------------------------
// one MultiMiMC7 absorption r <- r + x + E_r(x) (the body of k_eddsa_verify's hash)
__device__ __forceinline__ Fr ed_mimc7_absorb(const uint32_t* __restrict__ consts, const Fr& h, const Fr& x) {
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

// sign_mimc7 (mod.rs:210-236 on the real hash): request sk | randomness | message -> the record pk.x | pk.y | R.x | R.y | s | message
__global__ void __launch_bounds__(64) k_eddsa_sign(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const uint8_t* __restrict__ reqs,
                                                  size_t n, uint8_t* __restrict__ recs, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* req = reqs + g * 96;
  uint8_t* rec = recs + g * 192;
  bool good = true;
#pragma unroll 1
  for (int k = 0; k < 3; k++) good = good && canonical_fr(req + 32 * k);
  const Fr ca = ed_const(168700), cd = ed_const(168696);
  // the nonce r = MultiMiMC7([randomness, message]).  What a later step can read again (the message, sk) or rebuild (the nonce
  // from its words) is not kept in registers across the two products and the hashes.
  Fr h = Fr::zero();
#pragma unroll 1
  for (int k = 0; k < 2; k++) h = ed_mimc7_absorb(consts, h, fe_to_mont(fe_load<FrParams>(req + 32 + 32 * k)));
  uint32_t wn[8], wsk[8];
  fe_to_words(wn, fe_from_mont(h));
  fe_to_words(wsk, fe_load<FrParams>(req));
  EdPoint rp, pk;
  ed_mul_base<true>(tab, wn, wsk, rp, pk, ca, cd);
  // both points to affine by one inversion
  const Fr zi = fe_inv(fe_mul(rp.z, pk.z));
  const Fr rzi = fe_mul(zi, pk.z), pzi = fe_mul(zi, rp.z);
  const Fr rx = fe_mul(rp.x, rzi), ry = fe_mul(rp.y, rzi), px = fe_mul(pk.x, pzi), py = fe_mul(pk.y, pzi);
  h = Fr::zero();
#pragma unroll 1
  for (int k = 0; k < 5; k++) {
    const Fr x = k == 0 ? rx : k == 1 ? ry : k == 2 ? px : k == 3 ? py : fe_to_mont(fe_load<FrParams>(req + 64));
    h = ed_mimc7_absorb(consts, h, x);
  }
  const Fr s = ed_sign_s(fe_from_words<FrParams>(wn), fe_from_mont(h), fe_from_words<FrParams>(wsk));
  good = good && fe_lt_modulus(s);  // s >= r: the reference's "Invalid repr"
  if (good) {
    fe_store(rec, fe_from_mont(px));
    fe_store(rec + 32, fe_from_mont(py));
    fe_store(rec + 64, fe_from_mont(rx));
    fe_store(rec + 96, fe_from_mont(ry));
    fe_store(rec + 128, s);
    fe_store(rec + 160, fe_load<FrParams>(req + 64));
  } else {
    store_zeros(rec, 12);
  }
  ok[g] = good ? 1u : 0u;
}

// ---- launches --------------------------------------------------------------------------------------------------------------------
int eddsa_base_table(og_ctx* ctx, const uint8_t** tab) {
  if (!ctx->ed_tab_d) {
    uint8_t* t = nullptr;
    OG_HIP(hipMalloc((void**)&t, ED_TAB_BYTES));
    ctx->owned.push_back(t);
    hipLaunchKernelGGL(k_ed_table, dim3(1), dim3(ED_TAB_WINDOWS), 0, ctx->stream, t);
    OG_HIP(hipGetLastError());
    ctx->ed_tab_d = t;  // (the calls that read it are issued behind the build on the same stream)
  }
  *tab = ctx->ed_tab_d;
  return OG_OK;
}

int eddsa_pubkey(og_ctx* ctx, const uint8_t* sk_d, size_t n, uint8_t* pk_d, uint8_t* pkc_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  hipLaunchKernelGGL(k_eddsa_pubkey, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, tab, sk_d, n, pk_d, pkc_d, ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int eddsa_decompress(og_ctx* ctx, const uint8_t* in_d, size_t in_stride, size_t n, uint8_t* out_d, size_t out_stride, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  OG_REQUIRE(in_stride >= 32 && in_stride % 16 == 0 && out_stride % 16 == 0 && out_stride >= in_stride + 32, "eddsa_decompress: bad strides");
  hipLaunchKernelGGL(k_eddsa_decompress, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, in_d, in_stride, n, out_d, out_stride, ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int eddsa_sign(og_ctx* ctx, const uint8_t* requests_d, size_t n, uint8_t* records_d, uint32_t* ok_d) {
  if (n == 0) return OG_OK;
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  hipLaunchKernelGGL(k_eddsa_sign, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, tab, requests_d, n, records_d,
                     ok_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// ---- test seams (hooks builds only) --------------------------------------------------------------------------------------------------
#ifdef OG_AB_HOOKS
// the square-root routine alone, on arbitrary field elements: root of a (v = 1), canonical; ok = 0 and a zero root for a non-residue
// or a non-canonical a
__global__ void __launch_bounds__(64) k_hook_fr_sqrt(const uint8_t* __restrict__ a, size_t n, uint8_t* __restrict__ root, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Fr y;
  bool good = canonical_fr(a + g * 32);
  good = fr_sqrt_ratio(fe_to_mont(fe_load<FrParams>(a + g * 32)), Fr::one(), y) && good;
  if (good) fe_store(root + g * 32, fe_from_mont(y));
  else store_zeros(root + g * 32, 2);
  ok[g] = good ? 1u : 0u;
}

// the mod-ORDER step alone: triples r | h | sk (canonical) -> s as a 32-byte integer below ORDER, ok = 1 iff s < r
__global__ void __launch_bounds__(64) k_hook_ed_sign_s(const uint8_t* __restrict__ triples, size_t n, uint8_t* __restrict__ s_out, uint32_t* __restrict__ ok) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* t = triples + g * 96;
  const Fr s = ed_sign_s(fe_load<FrParams>(t), fe_load<FrParams>(t + 32), fe_load<FrParams>(t + 64));
  fe_store(s_out + g * 32, s);
  ok[g] = fe_lt_modulus(s) ? 1u : 0u;
}
#endif

}  // namespace og

#ifdef OG_AB_HOOKS
template <class Launch>
static int ed_hook_run(og_ctx* ctx, const char* what, bool args_ok, size_t n, uint32_t* ok_out, Launch&& launch) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && args_ok && ok_out && n >= 1 && n <= ((size_t)1 << 24), std::string(what) + ": bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    uint32_t* ok_d = nullptr;
    OG_TRY(arena_get(ctx, "eddsa.ok", n * 4, (void**)&ok_d));
    launch(ok_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipMemcpyAsync(ok_out, ok_d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}

extern "C" int og_hook_fr_sqrt_d(og_ctx* ctx, const uint8_t* a_d, size_t n, uint8_t* root_out_d, uint32_t* ok_out) {
  return ed_hook_run(ctx, "og_hook_fr_sqrt_d", a_d && root_out_d, n, ok_out, [&](uint32_t* ok_d) {
    hipLaunchKernelGGL(og::k_hook_fr_sqrt, dim3(og::grid_for(n, 64)), dim3(64), 0, ctx->stream, a_d, n, root_out_d, ok_d);
  });
}

extern "C" int og_hook_ed_sign_s_d(og_ctx* ctx, const uint8_t* triples_d, size_t n, uint8_t* s_out_d, uint32_t* ok_out) {
  return ed_hook_run(ctx, "og_hook_ed_sign_s_d", triples_d && s_out_d, n, ok_out, [&](uint32_t* ok_d) {
    hipLaunchKernelGGL(og::k_hook_ed_sign_s, dim3(og::grid_for(n, 64)), dim3(64), 0, ctx->stream, triples_d, n, s_out_d, ok_d);
  });
}
#endif
