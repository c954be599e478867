// Elementwise field kernels behind og_field_op_d / og_field_mulchain_d:
// the parity surface for Montgomery add/sub/mul/inv and the mulmod/s micro-benchmark.
#include "ctx.h"
#include "primitives.h"
#include "field.hip.h"
#include "field_w9.hip.h"

namespace og {

template <class M>
__global__ void __launch_bounds__(256) k_field_op(int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                 uint8_t* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<M> x = fe_to_mont(fe_load<M>(a + i * 32));
  Fe<M> y = op == 3 ? Fe<M>::zero() : fe_to_mont(fe_load<M>(b + i * 32));
  Fe<M> r;
  switch (op) {
    case 0: r = fe_add(x, y); break;
    case 1: r = fe_sub(x, y); break;
    case 2: r = fe_mul(x, y); break;
    default: r = x.is_zero() ? x : fe_inv(x); break;
  }
  fe_store(out + i * 32, fe_from_mont(r));
}

template <class M>
__global__ void __launch_bounds__(256) k_mulchain(uint8_t* __restrict__ x, const uint8_t* __restrict__ y, size_t n, int iters) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<M> a = fe_load<M>(x + i * 32);
  Fe<M> b = fe_load<M>(y + i * 32);
  for (int k = 0; k < iters; k++) a = fe_mul(a, b);
  fe_store(x + i * 32, a);
}

// The same chain with ONE element per wave in the w9 form (field_w9.hip.h): the limbs of x over nine lanes, y wave-uniform.
// Same Montgomery digits, so the same bytes as k_mulchain; *cycles = the longest wave's loop in shader cycles.
template <class M>
__global__ void __launch_bounds__(64) k_mulchain_w9(uint8_t* __restrict__ x, const uint8_t* __restrict__ y, size_t n, int iters,
                                                   unsigned long long* __restrict__ cycles) {
  const size_t i = blockIdx.x;
  const int lane = threadIdx.x;
  if (i >= n) return;
  const Fe<M> b = fe_load<M>(y + i * 32);
  U9 yu;
#pragma unroll
  for (int k = 0; k < 9; k++) yu.l[k] = OG_W9_FIRST(b.l[k]);
  const uint32_t nj = w9_modulus_limb<M>(lane);
  uint32_t xs = w9_spread(fe_load<M>(x + i * 32), lane);
  const unsigned long long t0 = OG_SHADER_CYCLES();
  for (int k = 0; k < iters; k++) xs = w9_mul<M>(yu, xs, nj);
  const unsigned long long t1 = OG_SHADER_CYCLES();
  const Fe<M> lazy = w9_collect<M>(xs);
  if (lane == 0) {
    fe_store(x + i * 32, fe_from_lazy_limbs<M>(lazy.l));
    if (cycles) atomicMax(cycles, t1 - t0);
  }
}

// the lane-local chain of one wave, timed the same way (the yardstick for the w9 form: n lanes of ONE wave)
template <class M>
__global__ void __launch_bounds__(64) k_mulchain_cycles(uint8_t* __restrict__ x, const uint8_t* __restrict__ y, size_t n, int iters,
                                                       unsigned long long* __restrict__ cycles) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<M> a = fe_load<M>(x + i * 32);
  const Fe<M> b = fe_load<M>(y + i * 32);
  const unsigned long long t0 = OG_SHADER_CYCLES();
  for (int k = 0; k < iters; k++) a = fe_mul(a, b);
  const unsigned long long t1 = OG_SHADER_CYCLES();
  fe_store(x + i * 32, a);
  if (cycles && (threadIdx.x & 63) == 0) atomicMax(cycles, t1 - t0);
}

int field_op(og_ctx* ctx, int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (n == 0) return OG_OK;
  dim3 g(grid_for(n, 256)), blk(256);
  if (field == 0)
    hipLaunchKernelGGL(k_field_op<FrParams>, g, blk, 0, ctx->stream, op, a, b, out, n);
  else
    hipLaunchKernelGGL(k_field_op<FqParams>, g, blk, 0, ctx->stream, op, a, b, out, n);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

int field_mulchain(og_ctx* ctx, int field, uint8_t* x, const uint8_t* y, size_t n, int iters, float* ms) {
  dim3 g(grid_for(n, 256)), blk(256);
  OG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  if (field == 0)
    hipLaunchKernelGGL(k_mulchain<FrParams>, g, blk, 0, ctx->stream, x, y, n, iters);
  else
    hipLaunchKernelGGL(k_mulchain<FqParams>, g, blk, 0, ctx->stream, x, y, n, iters);
  OG_HIP(hipGetLastError());
  OG_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  OG_HIP(hipEventSynchronize(ctx->ev1));
  OG_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return OG_OK;
}

// form 0: lane-local fe_mul, one lane per element (64-lane workgroups); form 1: w9, one wave per element
int field_mulchain_lat(og_ctx* ctx, int field, int form, uint8_t* x, const uint8_t* y, size_t n, int iters, float* ms, uint64_t* cycles_out) {
  unsigned long long* cyc = nullptr;
  OG_HIP(hipMalloc((void**)&cyc, 8));
  struct Free { void* p; ~Free() { (void)hipFree(p); } } fr{cyc};
  OG_HIP(hipMemsetAsync(cyc, 0, 8, ctx->stream));
  OG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  if (form == 1) {
    if (field == 0)
      hipLaunchKernelGGL(k_mulchain_w9<FrParams>, dim3((unsigned)n), dim3(64), 0, ctx->stream, x, y, n, iters, cyc);
    else
      hipLaunchKernelGGL(k_mulchain_w9<FqParams>, dim3((unsigned)n), dim3(64), 0, ctx->stream, x, y, n, iters, cyc);
  } else {
    if (field == 0)
      hipLaunchKernelGGL(k_mulchain_cycles<FrParams>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, x, y, n, iters, cyc);
    else
      hipLaunchKernelGGL(k_mulchain_cycles<FqParams>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, x, y, n, iters, cyc);
  }
  OG_HIP(hipGetLastError());
  OG_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  OG_HIP(hipEventSynchronize(ctx->ev1));
  OG_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  unsigned long long c = 0;
  OG_HIP(hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost));
  if (cycles_out) *cycles_out = c;
  return OG_OK;
}

}  // namespace og

#ifdef OG_AB_HOOKS
// ---- raw-limb seam of the hooks build (never in the shipped library, never in the header) ------------------------------------
// og_hook_fe_raw_d hands ONE routine of field.hip.h / ec.hip.h its operands AS LIMBS -- no fe_load, no fe_to_mont -- so that the
// lazy and weak operand bounds the routines document (limbs up to 2^30 / 2^31, values up to 42 N) reach the asm statements of
// mont_gfx950.inc on the hardware, and returns the routine's limbs untouched (tests/field_raw_cases.py holds the cases and the
// big-integer reference).  One kernel instantiation per (field, op): every asm statement gets a register allocation of its
// own.  Op numbers 0..8, 12, 13 are those of emu_fe_op and 64..70 those of emu_fq2_op (tests/hipemu/stubs.cpp); 37..41 and 71..74 are
// the forms of the single-Q addition (tests/field_rider_cases.py).
#include "ec.hip.h"
#include <mutex>

namespace og {

constexpr int RAW_SLOTS = 8, RAW_OUT = 2, RAW_NOPS = 80;

// Fe slots an op reads (0 = no such op).  Fq2 operands take two slots each (c0, c1).
constexpr int raw_arity(int op) {
  switch (op) {
    case 0: case 1: case 2: case 8: case 12: case 13: case 28: return 2;   // add sub mul eq sub_weak add2_weak add_lazy
    case 3: case 4: case 5: case 6: case 7: return 1;                        // sqr from_mont neg inv words
    case 20: return 3;                                                      // sqr_add(a, c, d)
    case 21: return 4;                                                      // mul_add(a, b, c, d)
    case 22: return 3;                                                      // mul_plus(a, b, c)
    case 23: return 5;                                                      // mul_add_plus(a, b, d, e, c)
    case 24: return 6;                                                      // mul_add3
    case 25: return 8;                                                      // mul_add4
    case 26: return 7;                                                      // sqr_add3
    case 27: case 29: case 30: case 31: case 33: case 34: case 35: case 36: return 1;  // dbl neg_lazy neg_lazy4 dbl_lazy weak_diff_is_zero canon lt_modulus to_mont
    case 32: return 3;                                                      // add3_weak
    case 37: case 40: return 2;                                             // sqr_plus(a, p)  rider4(a, b)
    case 38: return 4;                                                      // sqr_add_plus(a, c, d, p)
    case 39: case 41: return 1;                                             // neg_lazy6  norm_weak
    case 64: return 4;                                                      // Fq2 f_mul(a, b)
    case 65: return 2;                                                      // Fq2 f_sqr(a)
    case 66: return 8;                                                      // Fq2 f_mul_sub(a, b, c, d)
    case 67: case 68: case 69: case 70: return 6;                           // Fq2 f_sqr_sub(a, c, d)  f_mul_minus(a, b, x)  f_mul_minus_y(y, neg = 0 | 1, z, x)
    case 71: case 73: return 6;                                             // Fq2 f_mul_minus6(a, b, x)  f_sqr_rider(r, ppp, q)
    case 72: case 74: return 4;                                             // Fq2 f_mul_n4(a, b)  f_q_minus(q, x)
    default: return 0;
  }
}

template <class M>
constexpr bool raw_valid(int op) {
  return raw_arity(op) != 0 && (op < 64 || std::is_same<M, FqParams>::value);
}

template <class M>
OG_HD Fe<M> raw_flag(bool v) {
  Fe<M> r = Fe<M>::zero();
  r.l[0] = v ? 1u : 0u;
  return r;
}

template <class M, int OP>
OG_HD void fe_raw_apply(const Fe<M>* x, Fe<M>* o) {
  if constexpr (OP == 0) o[0] = fe_add(x[0], x[1]);
  else if constexpr (OP == 1) o[0] = fe_sub(x[0], x[1]);
  else if constexpr (OP == 2) o[0] = fe_mul(x[0], x[1]);
  else if constexpr (OP == 3) o[0] = fe_sqr(x[0]);
  else if constexpr (OP == 4) o[0] = fe_from_mont(x[0]);
  else if constexpr (OP == 5) o[0] = fe_neg(x[0]);
  else if constexpr (OP == 6) o[0] = fe_inv(x[0]);
  else if constexpr (OP == 7) {
    uint32_t w[8];
    fe_to_words(w, x[0]);
    o[0] = fe_from_words<M>(w);
  } else if constexpr (OP == 8) {
    o[0] = raw_flag<M>(x[0] == x[1]);
    o[0].l[1] = x[0].is_zero() ? 1u : 0u;
  } else if constexpr (OP == 12) o[0] = fe_sub_weak(x[0], x[1]);
  else if constexpr (OP == 13) o[0] = fe_add2_weak(x[0], x[1]);
  else if constexpr (OP == 20) o[0] = fe_sqr_add(x[0], x[1], x[2]);
  else if constexpr (OP == 21) o[0] = fe_mul_add(x[0], x[1], x[2], x[3]);
  else if constexpr (OP == 22) o[0] = fe_mul_plus(x[0], x[1], x[2]);
  else if constexpr (OP == 23) o[0] = fe_mul_add_plus(x[0], x[1], x[2], x[3], x[4]);
  else if constexpr (OP == 24) o[0] = fe_mul_add3(x[0], x[1], x[2], x[3], x[4], x[5]);
  else if constexpr (OP == 25) o[0] = fe_mul_add4(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
  else if constexpr (OP == 26) o[0] = fe_sqr_add3(x[0], x[1], x[2], x[3], x[4], x[5], x[6]);
  else if constexpr (OP == 27) o[0] = fe_dbl(x[0]);
  else if constexpr (OP == 28) o[0] = fe_add_lazy(x[0], x[1]);
  else if constexpr (OP == 29) o[0] = fe_neg_lazy(x[0]);
  else if constexpr (OP == 30) o[0] = fe_neg_lazy4(x[0]);
  else if constexpr (OP == 31) o[0] = fe_dbl_lazy(x[0]);
  else if constexpr (OP == 32) o[0] = fe_add3_weak(x[0], x[1], x[2]);
  else if constexpr (OP == 33) o[0] = raw_flag<M>(fe_weak_diff_is_zero(x[0]));
  else if constexpr (OP == 34) o[0] = fe_canon(x[0]);
  else if constexpr (OP == 35) o[0] = raw_flag<M>(fe_lt_modulus(x[0]));
  else if constexpr (OP == 36) o[0] = fe_to_mont(x[0]);
  else if constexpr (OP == 37) o[0] = fe_sqr_plus(x[0], x[1]);
  else if constexpr (OP == 38) o[0] = fe_sqr_add_plus(x[0], x[1], x[2], x[3]);
  else if constexpr (OP == 39) o[0] = fe_neg_lazy6(x[0]);
  else if constexpr (OP == 40) o[0] = fe_rider4(x[0], x[1]);
  else if constexpr (OP == 41) o[0] = fe_norm_weak(x[0]);
  else if constexpr (OP >= 64 && std::is_same<M, FqParams>::value) {
    const Fq2 a = {x[0], x[1]};
    Fq2 r;
    if constexpr (OP == 64) r = f_mul(a, Fq2{x[2], x[3]});
    else if constexpr (OP == 65) r = f_sqr(a);
    else if constexpr (OP == 66) r = f_mul_sub(a, Fq2{x[2], x[3]}, Fq2{x[4], x[5]}, Fq2{x[6], x[7]});
    else if constexpr (OP == 67) r = f_sqr_sub(a, Fq2{x[2], x[3]}, Fq2{x[4], x[5]});
    else if constexpr (OP == 68) r = f_mul_minus(a, Fq2{x[2], x[3]}, Fq2{x[4], x[5]});
    else if constexpr (OP == 69 || OP == 70) r = f_mul_minus_y(a, OP == 70, Fq2{x[2], x[3]}, Fq2{x[4], x[5]});
    else if constexpr (OP == 71) r = f_mul_minus6(a, Fq2{x[2], x[3]}, Fq2{x[4], x[5]});
    else if constexpr (OP == 72) r = f_mul_n4(a, Fq2{x[2], x[3]});
    else if constexpr (OP == 73) r = f_sqr_rider(a, Fq2{x[2], x[3]}, Fq2{x[4], x[5]});
    else r = f_q_minus(a, Fq2{x[2], x[3]});
    o[0] = r.c0;
    o[1] = r.c1;
  }
}

// one lane per case: in = n x 8 slots x 9 limbs (the slots the op reads; the rest is ignored), out = n x 2 x 9 limbs
template <class M, int OP>
__global__ void __launch_bounds__(64) k_fe_raw(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int NI = raw_arity(OP);
  Fe<M> x[NI], o[RAW_OUT];
#pragma unroll
  for (int s = 0; s < NI; s++)
#pragma unroll
    for (int k = 0; k < 9; k++) x[s].l[k] = in[i * (RAW_SLOTS * 9) + s * 9 + k];
  o[0] = Fe<M>::zero();
  o[1] = Fe<M>::zero();
  fe_raw_apply<M, OP>(x, o);
#pragma unroll
  for (int s = 0; s < RAW_OUT; s++)
#pragma unroll
    for (int k = 0; k < 9; k++) out[i * (RAW_OUT * 9) + s * 9 + k] = o[s].l[k];
}

typedef void (*RawLaunch)(hipStream_t, const uint32_t*, size_t, uint32_t*);

template <class M, int OP>
void raw_launch(hipStream_t st, const uint32_t* in, size_t n, uint32_t* out) {
  hipLaunchKernelGGL((k_fe_raw<M, OP>), dim3(grid_for(n, 64)), dim3(64), 0, st, in, n, out);
}

template <class M, int OP>
constexpr RawLaunch raw_pick() {
  if constexpr (raw_valid<M>(OP)) return &raw_launch<M, OP>;
  else return nullptr;
}

template <class M, int... OPS>
RawLaunch raw_lookup(int op, std::integer_sequence<int, OPS...>) {
  static const RawLaunch table[RAW_NOPS] = {raw_pick<M, OPS>()...};
  return op >= 0 && op < RAW_NOPS ? table[op] : nullptr;
}

}  // namespace og

extern "C" int og_hook_fe_raw_d(og_ctx* ctx, int field, int op, const uint32_t* operands_d, size_t n, uint32_t* out_d) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && operands_d && out_d && n >= 1 && n <= ((size_t)1 << 24) && (field == 0 || field == 1), "og_hook_fe_raw_d: bad argument");
    const RawLaunch f = field == 0 ? raw_lookup<FrParams>(op, std::make_integer_sequence<int, RAW_NOPS>{})
                                   : raw_lookup<FqParams>(op, std::make_integer_sequence<int, RAW_NOPS>{});
    OG_REQUIRE(f != nullptr, "og_hook_fe_raw_d: no such op in this field");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    f(ctx->stream, operands_d, n, out_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}
// ---- the group law driven alone, on raw limbs ---------------------------------------------------------------------------------
// og_hook_ec_chain_d walks one chain of additions per lane with NO normalisation in between and hands the accumulator back as
// limbs, weak x included, so that a test can start it from a non-canonical x (x + j N, up to the 5.5N the weak invariant of
// ec.hip.h allows) and see what the chain leaves.  acc: n x NC Fe (x, y, zz, zzz; NC = 4 for G1, 8 for G2) as 9 limbs each;
// steps: n x n_steps records of 1 + 8 x 9 words: kind (0 / 1: xyzz_madd_signed_w with q = slots 0.. and neg = kind; 2: xyzz_add_w
// with the XYZZ in slots 0..; 3: xyzz_norm), then the operand's Fe slots.  out: like acc.
namespace og {

constexpr int CHAIN_REC = 1 + 8 * 9;

template <class T> struct ChainIO;
template <> struct ChainIO<Fq> {
  static constexpr int NF = 1;
  OG_HD static Fq get(const uint32_t* p) {
    Fq r;
    for (int k = 0; k < 9; k++) r.l[k] = p[k];
    return r;
  }
  OG_HD static void put(uint32_t* p, const Fq& v) {
    for (int k = 0; k < 9; k++) p[k] = v.l[k];
  }
};
template <> struct ChainIO<Fq2> {
  static constexpr int NF = 2;
  OG_HD static Fq2 get(const uint32_t* p) { return {ChainIO<Fq>::get(p), ChainIO<Fq>::get(p + 9)}; }
  OG_HD static void put(uint32_t* p, const Fq2& v) {
    ChainIO<Fq>::put(p, v.c0);
    ChainIO<Fq>::put(p + 9, v.c1);
  }
};

template <class T>
__global__ void __launch_bounds__(64) k_ec_chain(const uint32_t* __restrict__ acc_in, const uint32_t* __restrict__ steps, size_t n, uint32_t n_steps,
                                                uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  typedef ChainIO<T> IO;
  constexpr int W = IO::NF * 9;  // words per coordinate
  const uint32_t* a = acc_in + i * 4 * W;
  XYZZ<T> acc = {IO::get(a), IO::get(a + W), IO::get(a + 2 * W), IO::get(a + 3 * W)};
#pragma unroll 1
  for (uint32_t s = 0; s < n_steps; s++) {  // one inlined site per primitive (ec.hip.h)
    const uint32_t* rec = steps + (i * n_steps + s) * CHAIN_REC;
    const uint32_t kind = rec[0];
    if (kind <= 1) acc = xyzz_madd_signed_w(acc, Affine<T>{IO::get(rec + 1), IO::get(rec + 1 + W)}, kind == 1);
    else if (kind == 2) acc = xyzz_add_w(acc, XYZZ<T>{IO::get(rec + 1), IO::get(rec + 1 + W), IO::get(rec + 1 + 2 * W), IO::get(rec + 1 + 3 * W)});
    else acc = xyzz_norm(acc);
  }
  uint32_t* o = out + i * 4 * W;
  IO::put(o, acc.x);
  IO::put(o + W, acc.y);
  IO::put(o + 2 * W, acc.zz);
  IO::put(o + 3 * W, acc.zzz);
}

}  // namespace og

extern "C" int og_hook_ec_chain_d(og_ctx* ctx, int g2, const uint32_t* acc_d, const uint32_t* steps_d, size_t n, uint32_t n_steps, uint32_t* out_d) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && acc_d && steps_d && out_d && n >= 1 && n <= ((size_t)1 << 16) && n_steps <= (1u << 16) && (g2 == 0 || g2 == 1),
               "og_hook_ec_chain_d: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    if (g2) hipLaunchKernelGGL(k_ec_chain<Fq2>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, acc_d, steps_d, n, n_steps, out_d);
    else hipLaunchKernelGGL(k_ec_chain<Fq>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, acc_d, steps_d, n, n_steps, out_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}
// ---- the wave-wide forms driven alone, on raw limbs ---------------------------------------------------------------------------
// og_hook_w9_raw_d hands ONE routine of field_w9.hip.h / mimc7.hip.h its operands as limbs, one 64-lane workgroup per case, and
// returns the result word of ALL 64 lanes (tests/w9_raw_cases.py holds the cases and the integer models).  in: n x 3 slots x 9 limbs,
// out: n x 5 words x 64 lanes.  Ops (a = slot 0 where it is the uniform operand):
//   0  w9_mul<M>(a, slot 1)                      one digit per wave, the element in lanes 0 .. 8
//   1  w9_mul<M, true, false>(a, slot 1 | 2)     a digit per row: slot 1 in row 0, slot 2 in row 1
//   2  w9_mul<M, true, true>                     the same with the 32-bit digit
//   3  w9_carry(slot 0 | 1)                      rows 0 | 1
//   4, 5, 6  w9_carry(w9_sub(slot 0, slot 1, w9_kn_limb<M, 4 | 8 | 16>))        (Fq, as the group law uses them)
//   7  w9_spread -> word 0, w9_collect -> fe_from_lazy_limbs -> word 1 (every row of 16 lanes gives its lanes' own copy)
//   8  w9_mimc7_round<2>(t = slot 0 in both rows) -> t2, t4, t6, t6r0, x       (Fr)
//   9  w9_mimc7_hash2<2>(l = slot 0, r = slot 1, lane-local) -> word 0 as in op 7      (Fr)
#include "ec_w9.hip.h"
#include "mimc7.hip.h"

namespace og {

constexpr int W9_SLOTS = 3, W9_OUTS = 5, W9_NOPS = 10;

template <class M>
constexpr bool w9_raw_valid(int op) {
  return op >= 0 && op < W9_NOPS && (op < 4 || op == 7 || (op < 7 ? std::is_same<M, FqParams>::value : std::is_same<M, FrParams>::value));
}

template <class M>
__device__ __forceinline__ Fe<M> w9_raw_fe(const uint32_t* p) {
  Fe<M> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = p[k];
  return r;
}

template <class M, int OP>
__global__ void __launch_bounds__(64) k_w9_raw(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out,
                                              const uint32_t* __restrict__ consts9) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  const int tid = threadIdx.x, rl = w9_row_limb(tid);
  const bool row1 = (tid & 16) != 0;
  const uint32_t* x = in + i * (W9_SLOTS * 9);
  uint32_t o[W9_OUTS] = {0u, 0u, 0u, 0u, 0u};
  if constexpr (OP == 0) {
    o[0] = w9_mul<M>(w9_gather(w9_const_limb(x, tid)), w9_const_limb(x + 9, tid), w9_modulus_limb<M>(tid));
  } else if constexpr (OP == 1 || OP == 2) {
    o[0] = w9_mul<M, true, OP == 2>(w9_gather(w9_const_limb(x, tid)), w9_const_limb(row1 ? x + 18 : x + 9, rl), w9_modulus_limb<M>(rl));
  } else if constexpr (OP == 3) {
    o[0] = w9_carry(w9_const_limb(row1 ? x + 9 : x, rl), rl);
  } else if constexpr (OP >= 4 && OP <= 6) {
    constexpr int K = OP == 4 ? 4 : OP == 5 ? 8 : 16;
    o[0] = w9_carry(w9_sub(w9_const_limb(x, tid), w9_const_limb(x + 9, tid), w9_kn_limb<M, K>(tid)), tid);
  } else if constexpr (OP == 7) {
    o[0] = w9_spread(w9_raw_fe<M>(x), tid);
    const Fe<M> c = w9_collect<M>(o[0]);
    o[1] = w9_const_limb(fe_from_lazy_limbs<M>(c.l).l, tid & 15);
  } else if constexpr (OP == 8) {
    w9_mimc7_round<2>(w9_const_limb(x, rl), w9_modulus_limb<M>(rl), row1, o[0], o[1], o[2], o[3], o[4]);
  } else {
    const Fr h = w9_mimc7_hash2<2>(consts9, w9_raw_fe<FrParams>(x), w9_raw_fe<FrParams>(x + 9), tid);
    o[0] = w9_const_limb(h.l, tid & 15);
  }
#pragma unroll
  for (int s = 0; s < W9_OUTS; s++) out[(i * W9_OUTS + s) * 64 + tid] = o[s];
}

typedef void (*W9RawLaunch)(hipStream_t, const uint32_t*, size_t, uint32_t*, const uint32_t*);

template <class M, int OP>
void w9_raw_launch(hipStream_t st, const uint32_t* in, size_t n, uint32_t* out, const uint32_t* consts9) {
  hipLaunchKernelGGL((k_w9_raw<M, OP>), dim3((unsigned)n), dim3(64), 0, st, in, n, out, consts9);
}

template <class M, int OP>
constexpr W9RawLaunch w9_raw_pick() {
  if constexpr (w9_raw_valid<M>(OP)) return &w9_raw_launch<M, OP>;
  else return nullptr;
}

template <class M, int... OPS>
W9RawLaunch w9_raw_lookup(int op, std::integer_sequence<int, OPS...>) {
  static const W9RawLaunch table[W9_NOPS] = {w9_raw_pick<M, OPS>()...};
  return op >= 0 && op < W9_NOPS ? table[op] : nullptr;
}

// og_hook_w9_ec_chain_d: one WAVE per chain of w9_xyzz_dbl / w9_xyzz_add (ec_w9.hip.h), nothing in between.  acc: n x 4 x 9 limbs
// (x, y, zz, zzz as the wave holds them: raw, spread); steps: n x n_steps records of 1 + 4 x 9 words -- kind 0: doubling; 1: addition
// of the operand in the record; 2: acc = the operand (the walk's first non-zero digit); 3: the kernel's exit (a strict product by
// one per coordinate, w9_collect, fe_from_lazy_limbs), the result spread again; 4: nothing (padding of a cut chain).
// out: n x 4 words x 64 lanes.
constexpr int W9_CHAIN_REC = 1 + 4 * 9;

__global__ void __launch_bounds__(64) k_w9_ec_chain(const uint32_t* __restrict__ acc_in, const uint32_t* __restrict__ steps, size_t n,
                                                   uint32_t n_steps, uint32_t* __restrict__ out) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const uint32_t nj = w9_modulus_limb<FqParams>(lane);
  const uint32_t* a = acc_in + i * 36;
  W9Pt acc = {w9_const_limb(a, lane), w9_const_limb(a + 9, lane), w9_const_limb(a + 18, lane), w9_const_limb(a + 27, lane)};
#pragma unroll 1
  for (uint32_t s = 0; s < n_steps; s++) {  // one inlined site per primitive; the kind is wave-uniform
    const uint32_t* rec = steps + (i * n_steps + s) * W9_CHAIN_REC;
    const uint32_t kind = rec[0];
    const W9Pt e = {w9_const_limb(rec + 1, lane), w9_const_limb(rec + 10, lane), w9_const_limb(rec + 19, lane), w9_const_limb(rec + 28, lane)};
    if (kind == 0) acc = w9_xyzz_dbl(acc, nj, lane);
    else if (kind == 1) acc = w9_xyzz_add(acc, e, nj, lane);
    else if (kind == 2) acc = e;
    else if (kind == 3) {
      const U9 one = w9_uniform(FqParams::ONE);
      const Fq ox = w9_collect<FqParams>(w9q_mul(one, acc.x, nj)), oy = w9_collect<FqParams>(w9q_mul(one, acc.y, nj));
      const Fq ozz = w9_collect<FqParams>(w9q_mul(one, acc.zz, nj)), ozzz = w9_collect<FqParams>(w9q_mul(one, acc.zzz, nj));
      acc = {w9_spread(fe_from_lazy_limbs<FqParams>(ox.l), lane), w9_spread(fe_from_lazy_limbs<FqParams>(oy.l), lane),
             w9_spread(fe_from_lazy_limbs<FqParams>(ozz.l), lane), w9_spread(fe_from_lazy_limbs<FqParams>(ozzz.l), lane)};
    }
  }
  uint32_t* o = out + i * 4 * 64;
  o[lane] = acc.x;
  o[64 + lane] = acc.y;
  o[128 + lane] = acc.zz;
  o[192 + lane] = acc.zzz;
}

}  // namespace og

extern "C" int og_hook_w9_raw_d(og_ctx* ctx, int field, int op, const uint32_t* operands_d, size_t n, uint32_t* out_d) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && operands_d && out_d && n >= 1 && n <= ((size_t)1 << 20) && (field == 0 || field == 1), "og_hook_w9_raw_d: bad argument");
    const W9RawLaunch f = field == 0 ? w9_raw_lookup<FrParams>(op, std::make_integer_sequence<int, W9_NOPS>{})
                                     : w9_raw_lookup<FqParams>(op, std::make_integer_sequence<int, W9_NOPS>{});
    OG_REQUIRE(f != nullptr, "og_hook_w9_raw_d: no such op in this field");
    OG_REQUIRE(ctx->mimc_consts9_d != nullptr, "og_hook_w9_raw_d: the context has no round constants");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    f(ctx->stream, operands_d, n, out_d, (const uint32_t*)ctx->mimc_consts9_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}

extern "C" int og_hook_w9_ec_chain_d(og_ctx* ctx, const uint32_t* acc_d, const uint32_t* steps_d, size_t n, uint32_t n_steps, uint32_t* out_d) {
  using namespace og;
  return guarded([&]() -> int {
    OG_REQUIRE(ctx && acc_d && steps_d && out_d && n >= 1 && n <= ((size_t)1 << 16) && n_steps <= (1u << 16), "og_hook_w9_ec_chain_d: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    OG_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_w9_ec_chain, dim3((unsigned)n), dim3(64), 0, ctx->stream, acc_d, steps_d, n, n_steps, out_d);
    OG_HIP(hipGetLastError());
    OG_HIP(hipStreamSynchronize(ctx->stream));
    return OG_OK;
  });
}
#endif  // OG_AB_HOOKS
