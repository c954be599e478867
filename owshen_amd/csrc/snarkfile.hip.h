// What the snarkjs-file layers share (zkey.hip: .zkey / .wtns / .r1cs, ptau.hip: .ptau): the iden3 binfile container, the
// decode / encode kernel for points stored as little-endian Montgomery numbers with R = 2^256, the DFT over group elements
// (both groups: the kernels are written once over the group law of ec.hip.h and stay free of out-of-line device calls,
// DESIGN.md 4.2), the host's Fr helpers and this library's / ffjavascript's roots of unity.  Included by those two
// translation units and, through point_spmv.hip.h, by groth16.hip (the evaluation form of the H query is a DFT over the key's
// points); everything here is a template or static.
#pragma once
#include "ctx.h"
#include "field.hip.h"
#include "ec.hip.h"
#include "key_blob.h"  // rd32 / rd64, the padded writer
#include <string.h>
#include <stdlib.h>
#include <map>
#include <vector>

namespace og {

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// a file coordinate v = x 2^256 mod q -> x in this library's Montgomery form: (v R)(2^-256 R) / R
OG_HD Fq lem_fix(const Fq& raw, const Fq& k) { return fe_mul(fe_to_mont(raw), k); }
OG_HD Fq2 lem_fix(const Fq2& raw, const Fq& k) { return {lem_fix(raw.c0, k), lem_fix(raw.c1, k)}; }
OG_HD bool lem_lt(const Fq& a) { return fe_lt_modulus(a); }
OG_HD bool lem_lt(const Fq2& a) { return fe_lt_modulus(a.c0) && fe_lt_modulus(a.c1); }
OG_HD uint32_t lem_or(const Fq& a) {
  uint32_t z = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) z |= a.l[i];
  return z;
}
OG_HD uint32_t lem_or(const Fq2& a) { return lem_or(a.c0) | lem_or(a.c1); }

// consts: K = 2^-256 (import) or 2^256 (export) in Montgomery form (32 B) | the curve's b in Montgomery form (T)
// flags[0] |= 1: a coordinate >= q;  |= 2: a point off the curve.  The point at infinity is all zeros on both sides.
// to_file = 0: file -> canonical (out_canon) and / or Montgomery (out_mont);  1: canonical -> file (out_canon)
template <class T>
__global__ void __launch_bounds__(256) k_lem_import(const uint8_t* __restrict__ in, size_t n, const uint8_t* __restrict__ consts,
                                                   uint8_t* __restrict__ out_canon, uint8_t* __restrict__ out_mont, uint32_t* __restrict__ flags,
                                                   int to_file) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<T> p = Affine<T>::load(in + i * Affine<T>::BYTES);
  Affine<T> c = Affine<T>::inf(), m = Affine<T>::inf();
  if (lem_or(p.x) | lem_or(p.y)) {
    if (!lem_lt(p.x) || !lem_lt(p.y)) {
      atomicOr(flags, 1u);
    } else {
      const Fq k = fe_load<FqParams>(consts);
      if (to_file) {  // x -> x 2^256 mod q, as a plain number
        m = {FieldIO<T>::to_mont(p.x), FieldIO<T>::to_mont(p.y)};
        c = {FieldIO<T>::from_mont(lem_fix(p.x, k)), FieldIO<T>::from_mont(lem_fix(p.y, k))};
      } else {
        m = {lem_fix(p.x, k), lem_fix(p.y, k)};
        c = {FieldIO<T>::from_mont(m.x), FieldIO<T>::from_mont(m.y)};
      }
      const T b = FieldIO<T>::load(consts + 32);
      if (!(f_sqr(m.y) == f_add(f_mul(f_sqr(m.x), m.x), b))) atomicOr(flags, 2u);
    }
  }
  if (out_canon) c.store(out_canon + i * Affine<T>::BYTES);
  if (out_mont) m.store(out_mont + i * Affine<T>::BYTES);
}

struct K256 {
  uint32_t l[8];
};
__device__ __forceinline__ K256 k256_load(const uint8_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
// k P: double-and-add from bit `top` down (253: every bit of a k < 2^254; up to 255 for any 256-bit k).  One site each of the doubling and the addition
// (ec.hip.h: inlined), in either group.
template <class T>
__device__ __forceinline__ XYZZ<T> ecntt_smul(const XYZZ<T>& p, const K256& k, int top = 253) {
  XYZZ<T> acc = XYZZ<T>::inf();
#pragma unroll 1
  for (int b = top; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((k.l[b >> 5] >> (b & 31)) & 1) acc = xyzz_add(acc, p);
  }
  return acc;
}

// x[i] = scale[i] . P_i (or P_i), affine Montgomery -> XYZZ
template <class T>
__global__ void __launch_bounds__(64) k_ecntt_load(const uint8_t* __restrict__ aff, size_t n, const uint8_t* __restrict__ scale, uint8_t* __restrict__ x) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  XYZZ<T> p = XYZZ<T>::from_affine(Affine<T>::load(aff + i * Affine<T>::BYTES));
  if (scale) p = ecntt_smul(p, k256_load(scale + i * 32));
  p.store(x + i * XYZZ<T>::BYTES);
}

// one decimation-in-frequency stage over points: (u, v) = (x[i], x[i + 2^s]) -> (u + v, tw[..] (u - v)); natural order in,
// bit-reversed order out after stages log_n - 1 .. 0.  tw[k] = w^k, canonical, k < n / 2.
template <class T>
__global__ void __launch_bounds__(64) k_ecntt_stage(uint8_t* __restrict__ x, int log_n, int s, const uint8_t* __restrict__ tw) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ((size_t)1 << (log_n - 1))) return;
  constexpr size_t PB = XYZZ<T>::BYTES;
  const size_t half = (size_t)1 << s, lo = t & (half - 1);
  const size_t i = ((t >> s) << (s + 1)) | lo, j = i + half;
  const XYZZ<T> u = XYZZ<T>::load(x + i * PB), v = XYZZ<T>::load(x + j * PB);
  const size_t k = lo << (log_n - 1 - s);
  if constexpr (XYZZ<T>::BYTES == 128) {  // G1: both results fit beside the multiplication (2 waves / SIMD)
    XYZZ<T> r[2];
#pragma unroll 1
    for (int op = 0; op < 2; op++) r[op] = xyzz_add(u, op ? xyzz_neg(v) : v);
    if (k) r[1] = ecntt_smul(r[1], k256_load(tw + k * 32));
    r[0].store(x + i * PB);
    r[1].store(x + j * PB);
  } else {  // G2: each result goes straight out -- a kept pair of XYZZ<Fq2> costs 624 B of scratch per lane, this form 112 B
#pragma unroll 1
    for (int op = 0; op < 2; op++) {
      XYZZ<T> w = xyzz_add(u, op ? xyzz_neg(v) : v);
      if (op && k) w = ecntt_smul(w, k256_load(tw + k * 32));
      w.store(x + (op ? j : i) * PB);
    }
  }
}

// position p holds X[rev(p)]: out[j] = scale[j] . X[j] (or X[j]) as affine bytes, j = rev(p) < n_out.  uniform: one scalar,
// scale[0], for every j.  mont = 0: canonical coordinates (a key's bytes); 1: Montgomery (more arithmetic follows on the device)
template <class T>
__global__ void __launch_bounds__(64) k_ecntt_finish(const uint8_t* __restrict__ x, int log_n, size_t n_out, const uint8_t* __restrict__ scale,
                                                    int uniform, uint8_t* __restrict__ out, int mont) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= ((size_t)1 << log_n)) return;
  const size_t j = log_n ? (size_t)(__brevll((unsigned long long)p) >> (64 - log_n)) : 0;
  if (j >= n_out) return;
  XYZZ<T> v = XYZZ<T>::load(x + p * XYZZ<T>::BYTES);
  if (scale) v = ecntt_smul(v, k256_load(scale + (uniform ? 0 : j * 32)));
  Affine<T> a = xyzz_to_affine(v);
  if (!mont) {
    a.x = FieldIO<T>::from_mont(a.x);
    a.y = FieldIO<T>::from_mont(a.y);
  }
  a.store(out + j * Affine<T>::BYTES);
}

// ---- host arithmetic (the field layer's own routines, on the host) ----------------------------------------------------------
static Fr zfr_load(const uint8_t* p) {
  uint32_t w[8];
  memcpy(w, p, 32);
  return fe_from_words<FrParams>(w);
}
static void zfr_store(uint8_t* p, const Fr& v) {  // v canonical
  uint32_t w[8];
  fe_to_words(w, v);
  memcpy(p, w, 32);
}
static Fr zfr_pow_words(const Fr& a, const uint32_t e[8]) {  // a in Montgomery form
  Fr r = Fr::one();
  for (int b = 255; b >= 0; b--) {
    r = fe_sqr(r);
    if ((e[b >> 5] >> (b & 31)) & 1) r = fe_mul(r, a);
  }
  return r;
}
static Fr zfr_pow2k(Fr a, int k) {  // a^(2^k)
  for (int i = 0; i < k; i++) a = fe_sqr(a);
  return a;
}
static bool zfr_is_one(const Fr& a) { return a == Fr::one(); }

// (r - 1) / 2^28, the odd cofactor (ntt.hip carries the same words)
static const uint32_t FR_T[8] = {0x3e1f593fu, 0x9b970914u, 0x833e8487u, 0x181585d2u, 0x85045b68u, 0x131a029bu, 0x0644e72eu, 0x00000003u};

struct FfRoots {
  bool ok = false;
  Fr w28_ff, w28_own;  // primitive 2^28-th roots, Montgomery: ffjavascript's nqr^T and this library's 7^T
};
// ffjavascript's F1Field takes the SMALLEST quadratic non-residue, counting up from 2, as the base of its roots of unity.
// For BN254's r that is 5 -- checked here, not remembered: g^T has order exactly 2^28 iff g is a non-residue.
static const FfRoots& ff_roots() {
  static const FfRoots roots = [] {
    FfRoots f;
    auto order_is_2_28 = [](uint32_t g, Fr* out) {
      const Fr w = zfr_pow_words(fe_to_mont(fe_from_u32<FrParams>(g)), FR_T);
      if (out) *out = w;
      return !zfr_is_one(zfr_pow2k(w, 27));
    };
    f.ok = !order_is_2_28(2, nullptr) && !order_is_2_28(3, nullptr) && order_is_2_28(5, &f.w28_ff) && order_is_2_28(7, &f.w28_own);
    return f;
  }();
  return roots;
}

// k (mod 2^log_n) with base^k = target, both of exact order 2^log_n
static uint64_t zfr_dlog_pow2(const Fr& base, const Fr& target, int log_n) {
  const Fr binv = fe_inv(base);
  uint64_t k = 0;
  Fr bk = Fr::one();  // binv^k
  Fr step = binv;     // binv^(2^b)
  for (int b = 0; b < log_n; b++) {
    const Fr t = fe_mul(target, bk);
    if (!zfr_is_one(zfr_pow2k(t, log_n - 1 - b))) {
      k |= 1ull << b;
      bk = fe_mul(bk, step);
    }
    step = fe_sqr(step);
  }
  return k;
}

static uint64_t inv_mod_pow2(uint64_t a, int log_n) {  // a odd
  uint64_t x = 1;
  for (int i = 0; i < 6; i++) x *= 2 - a * x;  // Newton: doubles the correct low bits
  return log_n >= 64 ? x : x & ((1ull << log_n) - 1);
}

// ---- containers ---------------------------------------------------------------------------------------------------------------
struct BinFile {
  uint32_t version = 0;
  std::map<uint32_t, std::pair<const uint8_t*, uint64_t>> sec;  // the first occurrence of every section id
};
static int binfile_parse(const uint8_t* p, size_t len, const char* magic, uint32_t max_version, const std::string& who, BinFile* out) {
  OG_REQUIRE(len >= 12 && memcmp(p, magic, 4) == 0, who + ": not a " + magic + " file");
  out->version = rd32(p + 4);
  OG_REQUIRE(out->version >= 1 && out->version <= max_version, who + ": unsupported version " + std::to_string(out->version));
  const uint32_t n_sec = rd32(p + 8);
  size_t off = 12;
  for (uint32_t k = 0; k < n_sec; k++) {
    OG_REQUIRE(off + 12 <= len, who + ": truncated section header");
    const uint32_t id = rd32(p + off);
    const uint64_t size = rd64(p + off + 4);
    off += 12;
    OG_REQUIRE(size <= len - off, who + ": section " + std::to_string(id) + " runs past the end of the file");
    out->sec.insert({id, {p + off, size}});
    off += size;
  }
  return OG_OK;
}

static const uint8_t FQ_BYTES[32] = {0x47, 0xfd, 0x7c, 0xd8, 0x16, 0x8c, 0x20, 0x3c, 0x8d, 0xca, 0x71, 0x68, 0x91, 0x6a, 0x81, 0x97,
                                     0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
static const uint8_t FR_BYTES[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                     0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

struct ZDev {  // hipMalloc'd scratch released on every exit path
  std::vector<void*> ptrs;
  ~ZDev() {
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

// K = 2^(+-256) mod q in Montgomery form | b of the curve in Montgomery form, as the kernels load them
static void lem_consts(bool g2, bool to_file, uint8_t out[32 + 64]) {
  Fq k = Fq::one();
  for (int i = 0; i < 256; i++) k = fe_dbl(k);
  if (!to_file) k = fe_inv(k);
  fe_store(out, k);
  const Fq three = fe_to_mont(fe_from_u32<FqParams>(3));
  if (!g2) {
    fe_store(out + 32, three);
    memset(out + 64, 0, 32);
  } else {  // b' = 3 / (9 + u)
    const Fq2 xi = {fe_to_mont(fe_from_u32<FqParams>(9)), Fq::one()};
    const Fq2 b = f_mul(Fq2{three, Fq::zero()}, f_inv(xi));
    fe_store(out + 32, b.c0);
    fe_store(out + 64, b.c1);
  }
}

// What the checked point kernels' host sides share: n points of one group up, the constants of lem_consts beside them, a
// zeroed flag word, ONE launch -- launch(in_d, consts_d, out_d, flags_d) -- and the flag word back, synchronised.  out: the
// kernel's n points to the host, or null; out_d: where they lie on the device, or null for scratch of this call.  What a raised
// flag means is the caller's business.
template <class Launch>
static int lem_run(og_ctx* ctx, ZDev& dev, bool g2, bool to_file, const uint8_t* in, size_t n, uint8_t* out, uint8_t* out_d, uint32_t* flags,
                   Launch launch) {
  const size_t pb = g2 ? 128 : 64;
  uint8_t *in_d, *c_d, *f_d;
  OG_TRY(dev.get(n * pb, &in_d));
  if (!out_d) OG_TRY(dev.get(n * pb, &out_d));
  OG_TRY(dev.get(96, &c_d));
  OG_TRY(dev.get(4, &f_d));
  alignas(16) uint8_t consts[96];
  lem_consts(g2, to_file, consts);
  OG_HIP(hipMemcpyAsync(in_d, in, n * pb, hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemcpyAsync(c_d, consts, 96, hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipMemsetAsync(f_d, 0, 4, ctx->stream));
  launch(in_d, c_d, out_d, (uint32_t*)f_d);
  OG_HIP(hipGetLastError());
  if (out) OG_HIP(hipMemcpyAsync(out, out_d, n * pb, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipMemcpyAsync(flags, f_d, 4, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

// file <-> canonical for `n` points of one group (host buffers in and out; `mont_d`, optional: the Montgomery copy stays on the device)
static int lem_convert(og_ctx* ctx, ZDev& dev, bool g2, bool to_file, const uint8_t* in, size_t n, uint8_t* out, uint8_t* mont_d,
                       const std::string& who) {
  if (n == 0) return OG_OK;
  uint32_t flags = 0;
  OG_TRY(lem_run(ctx, dev, g2, to_file, in, n, out, nullptr, &flags, [&](uint8_t* in_d, uint8_t* c_d, uint8_t* out_d, uint32_t* f_d) {
    if (g2)
      hipLaunchKernelGGL(k_lem_import<Fq2>, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in_d, n, c_d, out_d, mont_d, f_d, to_file ? 1 : 0);
    else
      hipLaunchKernelGGL(k_lem_import<Fq>, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in_d, n, c_d, out_d, mont_d, f_d, to_file ? 1 : 0);
  }));
  OG_REQUIRE(!(flags & 1), who + ": a point coordinate is not below the base-field modulus");
  OG_REQUIRE(!(flags & 2), who + ": a point is not on the curve");
  return OG_OK;
}

// DFT over points of one group (zkey.hip's head has the H-section use, ptau.hip's the Lagrange bases).  aff_mont_d: n = 2^log_n
// affine Montgomery points; tw: n / 2 canonical twiddles w^k; pre / post: optional canonical scalars applied before / after
// (post indexed by OUTPUT position: n of them, or ONE for every position if post_uniform); out_d: n_out affine points on the
// device, canonical or (mont) Montgomery.  Enqueues only: the caller synchronises before tw / pre / post die.
template <class T>
static int ecntt_run(og_ctx* ctx, ZDev& dev, const uint8_t* aff_mont_d, int log_n, const std::vector<uint8_t>& tw, const std::vector<uint8_t>* pre,
                     const std::vector<uint8_t>* post, bool post_uniform, size_t n_out, uint8_t* out_d, bool mont) {
  const size_t n = (size_t)1 << log_n;
  uint8_t *x_d, *tw_d, *pre_d = nullptr, *post_d = nullptr;
  OG_TRY(dev.get(n * XYZZ<T>::BYTES, &x_d));
  OG_TRY(dev.get(tw.size(), &tw_d));
  if (!tw.empty()) OG_HIP(hipMemcpyAsync(tw_d, tw.data(), tw.size(), hipMemcpyHostToDevice, ctx->stream));
  if (pre) {
    OG_TRY(dev.get(n * 32, &pre_d));
    OG_HIP(hipMemcpyAsync(pre_d, pre->data(), n * 32, hipMemcpyHostToDevice, ctx->stream));
  }
  if (post) {
    OG_TRY(dev.get(post->size(), &post_d));
    OG_HIP(hipMemcpyAsync(post_d, post->data(), post->size(), hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(k_ecntt_load<T>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, aff_mont_d, n, pre_d, x_d);
  OG_HIP(hipGetLastError());
  for (int s = log_n - 1; s >= 0; s--) {
    hipLaunchKernelGGL(k_ecntt_stage<T>, dim3(grid_for(n / 2, 64)), dim3(64), 0, ctx->stream, x_d, log_n, s, tw_d);
    OG_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_ecntt_finish<T>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, x_d, log_n, n_out, post_d, post_uniform ? 1 : 0, out_d,
                     mont ? 1 : 0);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// the G1 form with canonical points on the host (the .zkey H section, both ways)
static int ecntt_g1(og_ctx* ctx, ZDev& dev, const uint8_t* aff_mont_d, int log_n, const std::vector<uint8_t>& tw, const std::vector<uint8_t>* pre,
                    const std::vector<uint8_t>* post, size_t n_out, uint8_t* out) {
  uint8_t* out_d;
  OG_TRY(dev.get(((size_t)1 << log_n) * 64, &out_d));
  OG_TRY(ecntt_run<Fq>(ctx, dev, aff_mont_d, log_n, tw, pre, post, false, n_out, out_d, false));
  OG_HIP(hipMemcpyAsync(out, out_d, n_out * 64, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));  // (tw / pre / post: the host vectors outlive the copies)
  return OG_OK;
}

// powers of a Montgomery value as canonical bytes: out[k] = c a^k, k < count
static void pow_table(const Fr& a, const Fr& c, size_t count, std::vector<uint8_t>& out) {
  out.resize(count * 32);
  Fr t = c;
  for (size_t k = 0; k < count; k++) {
    zfr_store(&out[k * 32], fe_from_mont(t));
    t = fe_mul(t, a);
  }
}

static int blob_out(const std::vector<uint8_t>& v, uint8_t** out, size_t* len, const char* who) {
  uint8_t* a = static_cast<uint8_t*>(malloc(v.size() ? v.size() : 1));
  if (!a) {
    set_error(std::string(who) + ": out of host memory");
    return OG_ERR_INVALID;
  }
  memcpy(a, v.data(), v.size());
  *out = a;
  *len = v.size();
  return OG_OK;
}

}  // namespace og
