// The sparse matrix x vector product over POINTS: out_i = sum_e val[e] . base[idx[e]], a wire's entries summed level by level.
// ptau.hip builds a key's queries with it (the transposed QAP matrices over the Lagrange bases), groth16.hip folds C z into the
// L query at load (the transposed C over the DFT of the H query).  Templates and statics only, like snarkfile.hip.h.
#pragma once
#include "snarkfile.hip.h"
#include <algorithm>

namespace og {

static const uint32_t FR_ORDER_WORDS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static K256 fr_order_k256(uint32_t minus) {
  K256 k;
  memcpy(k.l, FR_ORDER_WORDS, 32);
  k.l[0] -= minus;  // (the low word is 0xf0000001: no borrow for minus <= 1)
  return k;
}

// terms[e] = val[e] . lag[idx[e]] (XYZZ); lag affine Montgomery, val canonical.  m1 = r - 1.
template <class T>
__global__ void __launch_bounds__(64) k_spmv_terms(const uint8_t* __restrict__ lag, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ val,
                                                  size_t nnz, K256 m1, uint8_t* __restrict__ terms) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  XYZZ<T> p = XYZZ<T>::from_affine(Affine<T>::load(lag + (size_t)idx[e] * Affine<T>::BYTES));
  const K256 k = k256_load(val + e * 32);
  uint32_t hi = 0, dm = 0;
  int top = -1;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    if (w) hi |= k.l[w];
    dm |= k.l[w] ^ m1.l[w];
    if (k.l[w]) top = 32 * w + 31 - __clz((int)k.l[w]);
  }
  if (dm == 0)
    p = xyzz_neg(p);
  else if (!(hi == 0 && k.l[0] == 1))
    p = ecntt_smul(p, k, top);  // every set bit, 255 included: [k]P = [k mod r]P, as og_setup reduces such a value (k = 0: no bit, infinity)
  p.store(terms + e * XYZZ<T>::BYTES);
}

// out[c] = sum of in[ptr[c] .. ptr[c + 1]) (an empty range: the point at infinity).  affine = 0: XYZZ out (another level
// follows); 1: canonical affine bytes (a query).
template <class T>
__global__ void __launch_bounds__(64) k_seg_sum(const uint8_t* __restrict__ in, const uint32_t* __restrict__ ptr, size_t n, uint8_t* __restrict__ out,
                                               int affine) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const uint32_t b = ptr[c], e = ptr[c + 1];
  XYZZ<T> acc = XYZZ<T>::inf();
#pragma unroll 1
  for (uint32_t i = b; i < e; i++) acc = xyzz_add(acc, XYZZ<T>::load(in + (size_t)i * XYZZ<T>::BYTES));
  if (!affine) {
    acc.store(out + c * XYZZ<T>::BYTES);
    return;
  }
  Affine<T> a = xyzz_to_affine(acc);
  a.x = FieldIO<T>::from_mont(a.x);
  a.y = FieldIO<T>::from_mont(a.y);
  a.store(out + c * Affine<T>::BYTES);
}

constexpr uint32_t SPMV_SEG = 32;  // terms one lane sums per level

// out_d[i] = sum over e in [tptr[i], tptr[i + 1]) of tval[e] . lag_d[tidx[e]], i < m: canonical affine, on the device
template <class T>
static int point_spmv(og_ctx* ctx, const uint8_t* lag_d, const std::vector<uint32_t>& tptr, const std::vector<uint32_t>& tidx,
                      const std::vector<uint8_t>& tval, size_t m, uint8_t* out_d) {
  const size_t nnz = tidx.size();
  ZDev dev;  // this product's scratch (terms, every level) goes back when it is done: the call's peak is its largest step
  uint8_t *idx_d, *val_d, *cur_d;
  OG_TRY(dev.get(nnz * 4, &idx_d));
  OG_TRY(dev.get(nnz * 32, &val_d));
  OG_TRY(dev.get(nnz * XYZZ<T>::BYTES, &cur_d));
  if (nnz) {
    OG_HIP(hipMemcpyAsync(idx_d, tidx.data(), nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    OG_HIP(hipMemcpyAsync(val_d, tval.data(), nnz * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_spmv_terms<T>, dim3(grid_for(nnz, 64)), dim3(64), 0, ctx->stream, lag_d, (const uint32_t*)idx_d, val_d, nnz, fr_order_k256(1), cur_d);
    OG_HIP(hipGetLastError());
  }
  // levels: while some wire still holds more than SPMV_SEG items, every run of SPMV_SEG items of a wire becomes one
  std::vector<std::vector<uint32_t>> keep;  // the host arrays outlive their copies
  std::vector<uint32_t> cp = tptr;
  for (;;) {
    uint32_t longest = 0;
    for (size_t i = 0; i < m; i++) longest = std::max(longest, cp[i + 1] - cp[i]);
    if (longest <= SPMV_SEG) break;
    std::vector<uint32_t> chunk, next(m + 1, 0);
    for (size_t i = 0; i < m; i++) {
      for (uint32_t s = cp[i]; s < cp[i + 1]; s += SPMV_SEG) chunk.push_back(s);
      next[i + 1] = (uint32_t)chunk.size();
    }
    const size_t n_chunks = chunk.size();
    chunk.push_back(cp[m]);  // the wires tile the items, so chunk c ends where chunk c + 1 starts -- in its own wire or at the next one
    uint8_t *p_d, *nxt_d;
    OG_TRY(dev.get((n_chunks + 1) * 4, &p_d));
    OG_TRY(dev.get(n_chunks * XYZZ<T>::BYTES, &nxt_d));
    keep.push_back(std::move(chunk));
    OG_HIP(hipMemcpyAsync(p_d, keep.back().data(), (n_chunks + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_seg_sum<T>, dim3(grid_for(n_chunks, 64)), dim3(64), 0, ctx->stream, cur_d, (const uint32_t*)p_d, n_chunks, nxt_d, 0);
    OG_HIP(hipGetLastError());
    cur_d = nxt_d;
    cp.swap(next);
  }
  uint8_t* p_d;
  OG_TRY(dev.get((m + 1) * 4, &p_d));
  OG_HIP(hipMemcpyAsync(p_d, cp.data(), (m + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_seg_sum<T>, dim3(grid_for(m, 64)), dim3(64), 0, ctx->stream, cur_d, (const uint32_t*)p_d, m, out_d, 1);
  OG_HIP(hipGetLastError());
  OG_HIP(hipStreamSynchronize(ctx->stream));
  return OG_OK;
}

}  // namespace og
