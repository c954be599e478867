// Batched witness generation for the withdraw circuit ("batched MiMC7 Merkle-path
// hashing for witness generation").  No reference counterpart: the snapshot's withdraw carries no
// circuit (/root/reference/src/services/api_services/withdraw.rs:27-71 is an ECDSA-authorised burn).
// The statement and its wire order are defined by oracle/py/withdraw.py (the spec) and mirrored by
// owshen_amd/circuit.py (the R1CS); this file fills the wires:
//
//   k_withdraw_core  one lane per proof: public inputs, the (4 + depth) MultiMiMC7 gadgets with every
//                    intermediate power (t^2, t^4, t^6, t^7 per round), the Merkle selectors
//   k_withdraw_pad   one lane per padding unit (a 3-wire gate or a 64-gate chained segment)
//   k_deposit_witness / k_split_core   the deposit and the split statement (further down), one lane per request
//   k_join_core      the join statement: two lanes per request, one per note
//   k_transfer_core / k_tw9_*   the transfer statement (near the end): one lane per request for batches, a permutation per wave in three
//                    launches for calls of at most 512 requests
//   k_claim_core     the claim statement (behind the wave-wide walks): one lane per request, whatever the size of the call -- x BASE walked
//                    projectively with its coordinates parked in the witness row, one inversion per request
//   k_send_core / k_redeem_core   the send and the redeem statement (behind claim): claim's walk of the key, then transfer's and split's back
//   k_sw9_* / k_jw9_*   the wave-wide walk of split and of join (at the end, behind transfer's, whose bodies they share): three launches
//                    each, for calls of at most 512 requests; k_split_core / k_join_core stay the form for batches
//
// Input record per proof, (8 + depth) x 32 B canonical LE:
//   nullifier | secret | amount | recipient | pad_seed | index (u64 in the low bytes) | token | chain_id | siblings[depth]
// (token and chain_id: the rest of what the reference's gate signs, /root/reference/contracts/src/Owshen.sol:69)
// Output: n_wires x 32 B canonical per proof, wire order as documented in oracle/py/withdraw.py.
#include "ctx.h"
#include "statements.h"
#include "mimc7.hip.h"
#include "host_fr4.h"
#include "field_w9.hip.h"
#include "eddsa.hip.h"
#include "primitives.h"
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>

namespace og {

__device__ __forceinline__ void lds_put9(uint32_t* p, const Fr& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) p[i] = v.l[i];
}
__device__ __forceinline__ Fr lds_get9(const uint32_t* p) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = p[i];
  return r;
}

constexpr int W_PUB = 6;
constexpr int W_REC = 8;  // fields of an input record before the siblings
// byte offsets of the record's fields
constexpr int W_NULLIFIER = 0, W_SECRET = 32, W_AMOUNT = 64, W_RECIPIENT = 96, W_PAD_SEED = 128, W_INDEX = 160, W_TOKEN = 192, W_CHAIN = 224;
constexpr int PAD_SEGMENT = 64;

struct WithdrawShape {
  uint64_t n_wires, n_constraints, first_gadget_wire, pad_base;
};

static WithdrawShape withdraw_shape(int depth, uint64_t n_pad3, uint64_t n_pad2) {
  WithdrawShape s;
  const uint64_t hashes = 4 + (uint64_t)depth;
  s.first_gadget_wire = 1 + W_PUB + 2 + 2 * (uint64_t)depth + 2;
  s.pad_base = s.first_gadget_wire + depth + hashes * 730 - 2;
  s.n_wires = s.pad_base + 3 * n_pad3 + 2 * n_pad2;
  s.n_constraints = 2 + 2 * (uint64_t)depth + hashes * 730 + n_pad3 + n_pad2;
  return s;
}

// CANON = true converts every wire out of Montgomery form as it is stored (the padding kernel: parallel, throughput
// bound); CANON = false stores the Montgomery value (the core kernel: one lane walks a proof's whole MiMC7 chain, so
// every multiplication taken off that chain is latency saved -- k_wires_from_mont converts afterwards, in parallel).
template <bool CANON>
struct WireWriterT {
  uint8_t* z;
  uint32_t w;
  __device__ __forceinline__ void put(uint32_t wire, const Fr& mont) { fe_store(z + (size_t)wire * 32, CANON ? fe_from_mont(mont) : mont); }
  __device__ __forceinline__ void push(const Fr& mont) { put(w++, mont); }
  // the same, by the lane of a pair that owns the wire (both lanes count)
  __device__ __forceinline__ void put_if(bool mine, uint32_t wire, const Fr& mont) { if (mine) put(wire, mont); }
  __device__ __forceinline__ void push_if(bool mine, const Fr& mont) { put_if(mine, w++, mont); }
};
typedef WireWriterT<true> WireWriter;

// One lane per proof.  The (4 + depth) MultiMiMC7 gadgets run through ONE inlined permutation body (rolled
// loops over gadgets, the two permutations of a gadget, and the 91 rounds): no device-function calls.
//
// PAIR: lanes 2g and 2g + 1 walk proof g together (mimc7.hip.h, the latency-bound form): per round both square t, the even lane
// forms t^4 and the odd lane t^3, they swap, then the even lane forms t^7 = t^4 t^3 -- the value the chain waits for -- while
// the odd lane forms the wire t^6 = t^4 t^2 beside it; the even lane stores t^2 and t^7, the odd lane t^4 and t^6.  Three
// multiplications deep instead of four, and half the stores on the chain.  One request's walk: 12 -> 9 ms.
template <bool PAIR>
__global__ void __launch_bounds__(64) k_withdraw_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs,
                                                     int depth, size_t n_wires, uint32_t first_gadget_wire, size_t n,
                                                     uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x, g = PAIR ? lane >> 1 : lane;
  const bool odd = PAIR && (threadIdx.x & 1), even = !odd;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(W_REC + depth) * 32;
  WireWriterT<false> ww{out + g * n_wires * 32, first_gadget_wire};
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(in + W_NULLIFIER));
  const Fr secret = fe_to_mont(fe_load<FrParams>(in + W_SECRET));
  const Fr amount = fe_to_mont(fe_load<FrParams>(in + W_AMOUNT));
  const Fr recipient = fe_to_mont(fe_load<FrParams>(in + W_RECIPIENT));
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + W_INDEX);
  const Fr token = fe_to_mont(fe_load<FrParams>(in + W_TOKEN));
  const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + W_CHAIN));
  ww.put_if(even, 0, Fr::one());
  ww.put_if(even, 3, recipient);
  ww.put_if(even, 4, amount);
  ww.put_if(even, 5, token);
  ww.put_if(even, 6, chain_id);
  ww.put_if(even, 7, nullifier);
  ww.put_if(even, 8, secret);
  for (int l = 0; l < depth; l++) {
    ww.put_if(even, 9 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + l) * 32)));
    ww.put_if(even, 9 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  ww.put_if(even, 9 + 2 * depth, fe_sqr(recipient));
  ww.put_if(even, 10 + 2 * depth, fe_sqr(chain_id));
  // gadget 0: inner = H(nullifier, secret); 1: asset = H(amount, token); 2: leaf = H(inner, asset);
  // 3: nullifier_hash = H(nullifier, 0) -> wire 2; gadget 4 + l: level l of the path, output -> next cur (wire 1 = root for
  // the last level)
  Fr cur = Fr::zero(), inner = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 4 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = nullifier; r_in = secret;
    } else if (h == 1) {
      l_in = amount; r_in = token;
    } else if (h == 2) {
      l_in = inner; r_in = cur;
    } else if (h == 3) {
      l_in = nullifier; r_in = Fr::zero(); out_wire = 2;
    } else {
      const int lvl = h - 4;
      const Fr sib = fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + lvl) * 32));
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push_if(even, l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    }
    // MultiMiMC7([l, r], key 0): k1 = l + E_0(l); out = k1 + r + E_k1(r), with E_k(x) = x_91 + k
    Fr k = Fr::zero(), x = l_in, k1 = Fr::zero();
#pragma unroll 1
    for (int p = 0; p < 2; p++) {
#pragma unroll 1
      for (int i = 0; i < MIMC7_ROUNDS; i++) {
        Fr t = fe_add3_weak(x, k, mimc7_const(consts, i));  // < 5N, only ever multiplied
        Fr t2 = PAIR ? OG_MIMC_LAT_SQR(t) : fe_sqr(t);
        if constexpr (PAIR) {  // (the latency forms of the products, field.hip.h: a request's walk is one wave waiting for itself)
          const Fr u = OG_MIMC_LAT_MUL(t2, pair_select(odd, t, t2));                    // even: t^4        odd: t^3
          const Fr v = pair_swap(u);                                           // even: t^3        odd: t^4
          const Fr y = OG_MIMC_LAT_MUL(pair_select(odd, v, u), pair_select(odd, t2, v));  // even: t^4 t^3    odd: t^4 t^2 = t^6
          x = pair_select(odd, pair_swap(y), y);                               // t^7 in both
          ww.put(ww.w + (odd ? 1 : 0), pair_select(odd, v, t2));               // t^2 | t^4
          ww.put(ww.w + (odd ? 2 : 3), y);                                     // t^7 | t^6
          ww.w += 4;
        } else {
          Fr t4 = fe_sqr(t2);
          Fr t6 = fe_mul(t4, t2);
          x = fe_mul(t6, t);
          ww.push(t2);
          ww.push(t4);
          ww.push(t6);
          ww.push(x);
        }
      }
      if (p == 0) {
        k1 = fe_add(l_in, x);
        ww.push_if(even, k1);
        k = k1;
        x = r_in;
      }
    }
    const Fr hout = fe_add(fe_add(fe_dbl(k1), r_in), x);
    if (out_wire < 0) ww.push_if(even, hout); else ww.put_if(even, (uint32_t)out_wire, hout);
    if (h == 0) inner = hout;
    if (h != 3) cur = hout;
  }
}

// ---- the walk of ONE request: a wave per proof (round 4) ------------------------------------------------------------------
// k_withdraw_core<true> gives a proof two lanes and walks its 36 hashes = 72 permutations one after the other: ~9.5 ms, the
// largest part of a single request.  The permutations are not all dependent:
//   * inner = H(nullifier, secret), asset = H(amount, token) and nullifier_hash = H(nullifier, 0) are independent of one
//     another (and the first permutation of the last, E_0(nullifier), IS the first of the first);
//   * MultiMiMC7([l, r]) = k1 + r + E_k1(r) with k1 = l + E_0(l): on a level where the path node is the RIGHT input, the first
//     permutation E_0(sibling) does not depend on the path at all.
// So a proof gets a whole wave, 32 lane pairs.  Phase A: pair 0 walks E_0(nullifier), pair 1 E_0(amount), pairs 2.. the
// E_0(sibling) of the levels whose path node is the right input; phase B: pairs 0 / 1 / 2 the second permutations of inner /
// asset / nullifier_hash, the remaining pairs the sibling jobs that did not fit phase A.  Every pair runs exactly one
// permutation per phase with one instruction stream (a pair without a job computes on zeros and stores nothing), results meet
// in LDS, and pair 0 goes on alone: leaf (2 permutations), then 2 permutations per left level and ONE per right level.
// 4 + depth + (number of left levels) permutations on the chain instead of 8 + 2 depth: 52 instead of 72 for a random leaf of a
// depth-32 tree (68 for leaf 0).  Every lane stores the wires of the permutations it walks, in the same places.
constexpr int WLAT_PAIRS = 32;
constexpr int WLAT_JOBS_A = WLAT_PAIRS - 2, WLAT_JOBS_B = WLAT_PAIRS - 3;  // sibling jobs per phase: 30 + 29 >= depth 59

__global__ void __launch_bounds__(64) k_withdraw_core_lat(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs, int depth,
                                                         size_t n_wires, uint32_t first_gadget_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  __shared__ uint32_t xch[64 + 4][9];  // k1 of sibling job j at [j]; [64] inner, [65] asset, [66] k1 of inner
  const size_t g = blockIdx.x;
  if (g >= n) return;
  const int lane = threadIdx.x, pair = lane >> 1;
  const bool odd = lane & 1, even = !odd;
  const uint8_t* in = inputs + g * (size_t)(W_REC + depth) * 32;
  uint8_t* z = out + g * n_wires * 32;
  auto put = [&](bool mine, uint32_t wire, const Fr& v) { if (mine) fe_store(z + (size_t)wire * 32, v); };
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + W_INDEX);
  // wire layout of a gadget (oracle/py/withdraw.py): [selector (path levels only)] | 364 wires of E_0 | k1 | 364 wires of E_k1 | out
  // gadgets 0..2 take 730 wires, nullifier_hash 729 (its output is a public wire), a path level 731 (the selector in front)
  auto gadget_base = [&](int h) -> uint32_t { return first_gadget_wire + (h < 4 ? (uint32_t)h * 730u : 2919u + 731u * (uint32_t)(h - 4)); };
  // the j-th level (ascending) whose path node is the RIGHT input, or -1
  auto right_level = [&](int j) -> int {
    int seen = 0;
    for (int l = 0; l < depth; l++)
      if ((index >> l) & 1) {
        if (seen == j) return l;
        seen++;
      }
    return -1;
  };
  // one permutation by this pair: E_k(x) over 91 rounds, the round wires stored at wbase (and, dup != 0, at dup as well)
  auto permute = [&](Fr x, const Fr& k, bool active, uint32_t wbase, uint32_t dup) -> Fr {
#pragma unroll 1
    for (int i = 0; i < MIMC7_ROUNDS; i++) {
      const Fr t = fe_add3_weak(x, k, mimc7_const(consts, i));
      const Fr t2 = fe_sqr(t);
      const Fr u = fe_mul(t2, pair_select(odd, t, t2));                        // even: t^4        odd: t^3
      const Fr v = pair_swap(u);                                               // even: t^3        odd: t^4
      const Fr y = fe_mul(pair_select(odd, v, u), pair_select(odd, t2, v));    // even: t^7        odd: t^6
      x = pair_select(odd, pair_swap(y), y);
      if (active) {
        const uint32_t w = wbase + 4u * (uint32_t)i;
        fe_store(z + (size_t)(w + (odd ? 1 : 0)) * 32, pair_select(odd, v, t2));  // t^2 | t^4
        fe_store(z + (size_t)(w + (odd ? 2 : 3)) * 32, y);                        // t^7 | t^6
        if (dup) {
          const uint32_t w2 = dup + 4u * (uint32_t)i;
          fe_store(z + (size_t)(w2 + (odd ? 1 : 0)) * 32, pair_select(odd, v, t2));
          fe_store(z + (size_t)(w2 + (odd ? 2 : 3)) * 32, y);
        }
      }
    }
    return x;
  };
  const Fr zero = Fr::zero();
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(in + W_NULLIFIER)), secret = fe_to_mont(fe_load<FrParams>(in + W_SECRET));
  const Fr amount = fe_to_mont(fe_load<FrParams>(in + W_AMOUNT)), recipient = fe_to_mont(fe_load<FrParams>(in + W_RECIPIENT));
  const Fr token = fe_to_mont(fe_load<FrParams>(in + W_TOKEN)), chain_id = fe_to_mont(fe_load<FrParams>(in + W_CHAIN));
  if (pair == 0) {  // the wires that are inputs or squares of inputs
    put(even, 0, Fr::one()); put(even, 3, recipient); put(even, 4, amount); put(even, 5, token); put(even, 6, chain_id);
    put(even, 7, nullifier); put(even, 8, secret);
    put(odd, 9 + 2 * depth, fe_sqr(recipient)); put(odd, 10 + 2 * depth, fe_sqr(chain_id));
  }
  for (int l = pair; l < depth; l += WLAT_PAIRS) {
    put(even, 9 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + l) * 32)));
    put(odd, 9 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  // ---------------- phase A ----------------
  Fr xa = zero;
  bool act = false;
  uint32_t wb = 0, dup = 0;
  int job = -1, lvl = -1;
  if (pair == 0) { xa = nullifier; act = true; wb = gadget_base(0); dup = gadget_base(3); }
  else if (pair == 1) { xa = amount; act = true; wb = gadget_base(1); }
  else {
    job = pair - 2;
    lvl = right_level(job);
    if (lvl >= 0) {
      xa = fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + lvl) * 32));
      act = true;
      wb = gadget_base(4 + lvl) + 1;
      put(even, gadget_base(4 + lvl), xa);  // the level's `left` selector wire: the sibling
    }
  }
  Fr k1 = fe_add(xa, permute(xa, zero, act, wb, dup));  // l + E_0(l)
  if (act) {
    put(even, wb + 364, k1);
    if (dup) put(odd, dup + 364, k1);
    if (even) lds_put9(xch[pair == 0 ? 66 : (pair == 1 ? 67 : job)], k1);
  }
  __syncthreads();
  // ---------------- phase B ----------------
  Fr xb = zero, kb = zero, rin = zero;
  act = false; wb = 0;
  int out_slot = -1;
  if (pair == 0) { xb = secret; rin = secret; kb = k1; act = true; wb = gadget_base(0) + 365; out_slot = 64; }
  else if (pair == 1) { xb = token; rin = token; kb = k1; act = true; wb = gadget_base(1) + 365; out_slot = 65; }
  else if (pair == 2) { xb = zero; rin = zero; kb = lds_get9(xch[66]); act = true; wb = gadget_base(3) + 365; }
  else {
    job = WLAT_JOBS_A + pair - 3;
    lvl = right_level(job);
    if (lvl >= 0) {
      xb = fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + lvl) * 32));
      act = true;
      wb = gadget_base(4 + lvl) + 1;
      put(even, gadget_base(4 + lvl), xb);
    }
  }
  const Fr xo = permute(xb, kb, act, wb, 0);
  if (pair <= 2) {  // second permutations: out = 2 k1 + r + x_91
    const Fr hout = fe_add(fe_add(fe_dbl(kb), rin), xo);
    if (pair == 2) put(even, 2, hout);                    // nullifier_hash: a public wire
    else {
      put(even, wb + 364, hout);
      if (even) lds_put9(xch[out_slot], hout);
    }
  } else if (act) {  // a late sibling job: k1 = l + E_0(l)
    const Fr k1b = fe_add(xb, xo);
    put(even, wb + 364, k1b);
    if (even) lds_put9(xch[job], k1b);
  }
  __syncthreads();
  if (pair != 0) return;
  // ---------------- the chain: pair 0 alone ----------------
  auto hash_rest = [&](const Fr& l_in, const Fr& r_in, bool have_k1, const Fr& k1_in, uint32_t base, int out_wire) -> Fr {
    Fr kk = k1_in;
    if (!have_k1) {
      kk = fe_add(l_in, permute(l_in, zero, true, base, 0));
      put(even, base + 364, kk);
    }
    const Fr xr = permute(r_in, kk, true, base + 365, 0);
    const Fr h = fe_add(fe_add(fe_dbl(kk), r_in), xr);
    put(even, out_wire >= 0 ? (uint32_t)out_wire : base + 729, h);
    return h;
  };
  Fr cur = hash_rest(lds_get9(xch[64]), lds_get9(xch[65]), false, zero, gadget_base(2), -1);  // leaf = H(inner, asset)
  int rj = 0;
#pragma unroll 1
  for (int l = 0; l < depth; l++) {
    const uint32_t gb = gadget_base(4 + l);
    const int out_wire = l == depth - 1 ? 1 : -1;
    if ((index >> l) & 1) {  // the path node is the right input: E_0(sibling) and the selector wire are already there
      cur = hash_rest(zero, cur, true, lds_get9(xch[rj]), gb + 1, out_wire);
      rj++;
    } else {
      const Fr sib = fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + l) * 32));
      put(even, gb, cur);  // `left` selector wire: the path node
      cur = hash_rest(cur, sib, false, zero, gb + 1, out_wire);
    }
  }
}

// ---- the walk in the wave-wide form (round 6; calls of at most 512 requests): ONE permutation per wave, three launches -----------------------------------------------
// field_w9.hip.h: a Montgomery product with its nine limbs in nine lanes is 616 cycles on a lone wave against 904 for the lane-local
// one, and in that form a round's additions, constant and stores are ONE instruction each instead of nine: a MiMC7 round -- t = x +
// k + c, four products (t^2, t^4, t^6, t^7), four stores -- is ~2 600 cycles against the lane pair's ~3 400; and with a second row of
// the wave as the lane group for the pair's t^3 || t^4 (ROWS: mimc7.hip.h w9_mimc7_round, the form the launches use) it is three
// products deep, t^6 computed beside t^7.  A wave holds one permutation, so the independent permutations of a proof (what
// k_withdraw_core_lat gives its 32 lane pairs) become one-wave WORKGROUPS that land on different CUs, in three launches:
//   k_w9_first   grid n x (3 + depth): E_0(nullifier) (wires of gadgets 0 and 3), E_0(amount), E_0(sibling_l) of every level whose path
//                node is the RIGHT input, and one workgroup for the wires that are inputs or squares of inputs
//   k_w9_second  grid n x 3: the second permutations of inner = H(nullifier, secret), asset = H(amount, token), nullifier_hash
//   k_w9_chain   grid n: leaf = H(inner, asset), then per level two permutations (left) or one (right): 4 + depth + #left on the chain
// Values pass between the launches as nine lazy limbs (xch).  Wires are stored as nine limbs too (36 B, one store instruction per
// wire: wl) and k_wires_from_limbs takes them to the canonical 32 bytes afterwards, in parallel -- where k_wires_from_mont takes
// the other kernels' 32-byte Montgomery values.  Bounds (multiples of N; the strict products accept limbs < 2^31 and a b < 169 N^2):
// forms 0 and 1: x < 2, c < 2, key k1 = l + x_91 < 4  =>  t < 8, t^2 .. t^7 fine (t^6 t: 2 x 8); a hash's output 2 k1 + r + x_91 < 12
// is carried and multiplied by one (< 2 again, limbs < 2^29 + 32) before it is anybody's input.  Form 2 (the 32-bit digit: what runs):
// mimc7.hip.h w9_mimc7_round -- x < 8.5, k1 < 10.5, t < 21, a hash's output < 32, through the same STRICT product by one: < 2.
constexpr int W9_XCH = 8;  // xch slots per proof beyond the levels: [depth + 0] k1 of inner / nullifier_hash, [1] k1 of asset, [2] inner, [3] asset,
                           // [4 .. 7]: 36 words nobody reads -- where the lanes without a limb store (w9_permute `dump`)
// `tid` = threadIdx.x (row 0 stores); `lane` = the limb a lane holds (w9_row_limb(tid) with ROWS -- rows 0 and 1 load --, tid without)
__device__ __forceinline__ void w9_store(uint32_t* wl, uint32_t wire, uint32_t v, int tid) { if (tid < 9) wl[(size_t)wire * 9 + tid] = v; }
__device__ __forceinline__ uint32_t w9_load(const uint32_t* p, int lane) { return lane < 9 ? p[lane] : 0u; }
// E_k(x) without the final + k: 91 rounds, the round wires at wbase (and at dup, if non-zero)
// With rows, a round's four wires leave in TWO store instructions: row 0 holds t^2 and t^4, row 1 t^6 and t^7 (w9_mimc7_round), the
// four wires are 36 consecutive words, so lane (row, limb) points at word 18 row + limb of the round's block, stores once there and
// once nine words on (a vector store costs a lone wave its address pass whether nine lanes are active or eighteen).
// The stores are UNCONDITIONAL -- lanes without a limb write a dump word (`dump`: a spare xch slot of the proof) -- because a store
// behind a branch makes the compiler wait for ALL memory operations before the next round's constant is used (vmcnt(0): the
// count is unknown on the path around the branch), i.e. for the stores' own completion, every round; without the branch the
// wait is for the constant alone (asked for a round ahead: mimc7.hip.h w9_mimc7_rounds) and the stores drain under the products.
template <int FORM, bool DUP>
__device__ __forceinline__ uint32_t w9_permute(const uint32_t* __restrict__ consts9, uint32_t x, uint32_t k, uint32_t nj, int tid, int lane,
                                               uint32_t* __restrict__ wl, uint32_t wbase, uint32_t dup, uint32_t* __restrict__ dump) {
  const int cl = lane < 15 ? lane : 15;
  const bool row1 = (tid & 16) != 0;
  const bool stores = FORM ? lane < 9 : tid < 9;
  const uint32_t off = (uint32_t)(lane < 9 ? lane : 0) + (FORM && row1 ? 18u : 0u);
  uint32_t* p = stores ? wl + (size_t)wbase * 9 + off : dump;
  uint32_t* pd = stores ? wl + (size_t)dup * 9 + off : dump;
  const ptrdiff_t step = stores ? 36 : 0;
  uint32_t c = consts9[cl];
#pragma unroll 1
  for (int i = 0; i < MIMC7_ROUNDS; i++, p += step, pd += step) {
    const uint32_t c_next = consts9[(i + 1 < MIMC7_ROUNDS ? i + 1 : i) * 16 + cl];
    uint32_t t2, t4, t6, t6r0;
    w9_mimc7_round<FORM>(x + k + c, nj, row1, t2, t4, t6, t6r0, x);
    c = c_next;
    if (FORM) {
      const uint32_t s0 = row1 ? t6r0 : t2, s1 = row1 ? t6 : t4;  // row 0: wires w, w + 1 = t^2, t^4; row 1: w + 2, w + 3 = t^6, t^7
      p[0] = s0; p[9] = s1;
      if (DUP) { pd[0] = s0; pd[9] = s1; }
    } else {
      p[0] = t2; p[9] = t4; p[18] = t6; p[27] = x;
      if (DUP) { pd[0] = t2; pd[9] = t4; pd[18] = t6; pd[27] = x; }
    }
  }
  return x;
}
// a sum of a few elements (limbs < 2^32, value < 169 N) -> the same value mod N below 2 N with limbs < 2^29 + 32
__device__ __forceinline__ uint32_t w9_renorm(uint32_t v, uint32_t nj, int lane) {
  return w9_mul<FrParams>(w9_uniform(FrParams::ONE), w9_carry(v, lane), nj);
}
__device__ __forceinline__ uint32_t w9_gadget_base(uint32_t fgw, int h) { return fgw + (h < 4 ? (uint32_t)h * 730u : 2919u + 731u * (uint32_t)(h - 4)); }
__device__ __forceinline__ void w9_put_fe(uint32_t* wl, uint32_t wire, const Fr& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) wl[(size_t)wire * 9 + i] = v.l[i];
}

template <int FORM>
__global__ void __launch_bounds__(64) k_w9_first(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_core,
                                                uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int jobs = 3 + depth, tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / jobs;
  const int job = (int)(blockIdx.x % jobs);
  const uint8_t* in = inputs + g * (size_t)(W_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_core * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + W9_XCH) * 9;
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + W_INDEX);
  if (job == 2 + depth) {  // the wires that are inputs or squares of inputs: lane-local values, a lane per wire
    const int lane = tid;
    const Fr recipient = fe_to_mont(fe_load<FrParams>(in + W_RECIPIENT)), chain_id = fe_to_mont(fe_load<FrParams>(in + W_CHAIN));
    if (lane == 0) w9_put_fe(wl, 0, Fr::one());
    if (lane == 1) w9_put_fe(wl, 3, recipient);
    if (lane == 2) w9_put_fe(wl, 4, fe_to_mont(fe_load<FrParams>(in + W_AMOUNT)));
    if (lane == 3) w9_put_fe(wl, 5, fe_to_mont(fe_load<FrParams>(in + W_TOKEN)));
    if (lane == 4) w9_put_fe(wl, 6, chain_id);
    if (lane == 5) w9_put_fe(wl, 7, fe_to_mont(fe_load<FrParams>(in + W_NULLIFIER)));
    if (lane == 6) w9_put_fe(wl, 8, fe_to_mont(fe_load<FrParams>(in + W_SECRET)));
    if (lane == 7) w9_put_fe(wl, 9 + 2 * depth, fe_sqr(recipient));
    if (lane == 8) w9_put_fe(wl, 10 + 2 * depth, fe_sqr(chain_id));
    for (int l = lane; l < depth; l += 64) {
      w9_put_fe(wl, 9 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + l) * 32)));
      w9_put_fe(wl, 9 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
    }
    return;
  }
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const uint8_t* src = in + W_NULLIFIER;  // job 0
  uint32_t wbase = w9_gadget_base(fgw, 0), dup = w9_gadget_base(fgw, 3);
  int slot = depth;
  if (job == 1) { src = in + W_AMOUNT; wbase = w9_gadget_base(fgw, 1); dup = 0; slot = depth + 1; }
  if (job >= 2) {
    const int lvl = job - 2;
    if (!((index >> lvl) & 1)) return;  // the path node is the LEFT input of this level: its first permutation is the chain's
    src = in + (size_t)(W_REC + lvl) * 32;
    wbase = w9_gadget_base(fgw, 4 + lvl) + 1;
    dup = 0;
    slot = lvl;
  }
  const uint32_t l_in = w9_spread(fe_to_mont(fe_load<FrParams>(src)), lane);
  if (job >= 2) w9_store(wl, wbase - 1, l_in, tid);  // the level's `left` selector wire: the sibling
  uint32_t* dump = xch + (size_t)(depth + 4) * 9;
  const uint32_t k1 = l_in + (dup ? w9_permute<FORM, true>(consts9, l_in, 0u, nj, tid, lane, wl, wbase, dup, dump)
                                  : w9_permute<FORM, false>(consts9, l_in, 0u, nj, tid, lane, wl, wbase, 0u, dump));  // l + E_0(l): < 4 N (form 2: < 10.5 N, mimc7.hip.h), lazy limbs
  w9_store(wl, wbase + 364, k1, tid);
  if (dup) w9_store(wl, dup + 364, k1, tid);
  if (tid < 9) xch[(size_t)slot * 9 + lane] = k1;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_w9_second(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_core,
                                                 uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 3;
  const int job = (int)(blockIdx.x % 3);  // 0 inner, 1 asset, 2 nullifier_hash
  const uint8_t* in = inputs + g * (size_t)(W_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_core * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + W9_XCH) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const uint32_t k1 = w9_load(xch + (size_t)(depth + (job == 1 ? 1 : 0)) * 9, lane);
  uint32_t r_in = 0;
  if (job == 0) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + W_SECRET)), lane);
  if (job == 1) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + W_TOKEN)), lane);
  const uint32_t base = w9_gadget_base(fgw, job == 2 ? 3 : job);
  const uint32_t xr = w9_permute<FORM, false>(consts9, r_in, k1, nj, tid, lane, wl, base + 365, 0u, xch + (size_t)(depth + 4) * 9);
  const uint32_t hout = w9_renorm(2u * k1 + r_in + xr, nj, lane);
  if (job == 2) { w9_store(wl, 2, hout, tid); return; }  // nullifier_hash: a public wire
  w9_store(wl, base + 729, hout, tid);
  if (tid < 9) xch[(size_t)(depth + 2 + job) * 9 + lane] = hout;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_w9_chain(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_core,
                                                uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x;
  const uint8_t* in = inputs + g * (size_t)(W_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_core * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + W9_XCH) * 9;
  uint32_t* dump = xch + (size_t)(depth + 4) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + W_INDEX);
  // H(l, r) from its first permutation on (have_k1: that one is already there), wires at base; the output below 2 N
  auto hash_rest = [&](uint32_t l_in, uint32_t r_in, bool have_k1, uint32_t k1, uint32_t base, int out_wire) -> uint32_t {
    if (!have_k1) {
      k1 = l_in + w9_permute<FORM, false>(consts9, l_in, 0u, nj, tid, lane, wl, base, 0u, dump);
      w9_store(wl, base + 364, k1, tid);
    }
    const uint32_t xr = w9_permute<FORM, false>(consts9, r_in, k1, nj, tid, lane, wl, base + 365, 0u, dump);
    const uint32_t h = w9_renorm(2u * k1 + r_in + xr, nj, lane);
    w9_store(wl, out_wire >= 0 ? (uint32_t)out_wire : base + 729, h, tid);
    return h;
  };
  uint32_t cur = hash_rest(w9_load(xch + (size_t)(depth + 2) * 9, lane), w9_load(xch + (size_t)(depth + 3) * 9, lane), false, 0u,
                           w9_gadget_base(fgw, 2), -1);  // leaf = H(inner, asset)
#pragma unroll 1
  for (int l = 0; l < depth; l++) {
    const uint32_t gb = w9_gadget_base(fgw, 4 + l);
    const int out_wire = l == depth - 1 ? 1 : -1;
    if ((index >> l) & 1) {  // the path node is the right input: E_0(sibling), k1 and the selector wire are k_w9_first's
      cur = hash_rest(0u, cur, true, w9_load(xch + (size_t)l * 9, lane), gb + 1, out_wire);
    } else {
      w9_store(wl, gb, cur, tid);  // `left` selector wire: the path node
      cur = hash_rest(cur, w9_spread(fe_to_mont(fe_load<FrParams>(in + (size_t)(W_REC + l) * 32)), lane), false, 0u, gb + 1, out_wire);
    }
  }
}

// wires [0, n_core) of every proof: nine lazy Montgomery limbs (what the w9 kernels left in wl) -> canonical 32 bytes in z
__global__ void __launch_bounds__(256) k_wires_from_limbs(const uint32_t* __restrict__ wl, uint8_t* __restrict__ out, size_t n_wires, uint32_t n_core) {
  OG_FILLER_PRIO();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_core) return;
  const uint32_t* p = wl + ((size_t)blockIdx.y * n_core + i) * 9;
  uint32_t t[9];
#pragma unroll
  for (int k = 0; k < 9; k++) t[k] = p[k];
  Fr o = Fr::zero();
  o.l[0] = 1;
  fe_store(out + ((size_t)blockIdx.y * n_wires + i) * 32, fe_canon(fe_mul(fe_from_lazy_limbs<FrParams>(t), o)));
}

// wires [0, n_core) of every proof: Montgomery -> canonical (what k_withdraw_core left behind)
// mult = 1: the kernels' form (x 2^261); mult = 32: the host walk's form (x 2^256: stored * 2^5 * 2^-261 = stored / 2^256)
__global__ void __launch_bounds__(256) k_wires_from_mont(uint8_t* __restrict__ out, size_t n_wires, uint32_t n_core, uint32_t mult) {
  OG_FILLER_PRIO();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_core) return;
  uint8_t* p = out + ((size_t)blockIdx.y * n_wires + i) * 32;
  Fr o = Fr::zero();
  o.l[0] = mult;
  fe_store(p, fe_canon(fe_mul(fe_load<FrParams>(p), o)));
}

// x = seed + wire; v = x^5; boolean parity wire when wire % 5 == 0.  Returns Montgomery form.
__device__ __forceinline__ Fr pad_value(const Fr& seed_canon, uint32_t wire) {
  Fr x = fe_to_mont(fe_add(seed_canon, fe_from_u32<FrParams>(wire)));
  Fr x2 = fe_sqr(x);
  Fr v = fe_mul(fe_sqr(x2), x);
  if (wire % 5 == 0) {
    Fr c = fe_from_mont(v);
    return (c.l[0] & 1) ? Fr::one() : Fr::zero();
  }
  return v;
}

__global__ void __launch_bounds__(256) k_withdraw_pad(const uint8_t* __restrict__ inputs, int depth, size_t n_wires, uint32_t pad_base,
                                                     uint32_t n_pad3, uint32_t n_pad2, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const uint32_t n_seg = (n_pad2 + PAD_SEGMENT - 1) / PAD_SEGMENT;
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_pad3 + n_seg) return;
  const size_t g = blockIdx.y;
  const Fr seed = fe_load<FrParams>(inputs + g * (size_t)(W_REC + depth) * 32 + W_PAD_SEED);
  WireWriter ww{out + g * n_wires * 32, 0};
  const Fr one = Fr::one(), two = fe_dbl(one);
  if (u < n_pad3) {
    ww.w = pad_base + 3 * u;
    Fr p = pad_value(seed, ww.w), q = pad_value(seed, ww.w + 1);
    ww.push(p);
    ww.push(q);
    ww.push(fe_mul(fe_add(p, one), fe_add(q, two)));
  } else {
    const uint32_t s = u - n_pad3;
    const uint32_t g0 = s * PAD_SEGMENT, g1 = g0 + PAD_SEGMENT < n_pad2 ? g0 + PAD_SEGMENT : n_pad2;
    ww.w = pad_base + 3 * n_pad3 + 2 * g0;
    Fr prev = one;  // the constant-one wire
    for (uint32_t k = g0; k < g1; k++) {
      Fr p = pad_value(seed, ww.w);
      ww.push(p);
      prev = fe_mul(fe_add(p, one), fe_add(prev, two));
      ww.push(prev);
    }
  }
}

// Boundary check of the input records (they arrive from HTTP: /root/reference/src/services/api_services/withdraw.rs:15-19):
// every field element must be the canonical encoding (< r) -- a value >= r would be reduced silently, i.e. two encodings of one
// nullifier -- and the index must fit the tree (u64 in the low bytes, < 2^depth, upper bytes zero: the circuit reads only its low
// `depth` bits).  That recipient and token are 160-bit addresses is the gate contract's check (contracts/OwshenWithdrawGate.sol):
// the statement itself takes any field element.  bad[g] = lowest offending field of record g (atomicMin;
// the caller initialises it to 0xffffffff): 0 nullifier, 1 secret, 2 amount, 3 recipient, 4 pad_seed, 5 index, 6 token,
// 7 chain_id, 8 + l sibling l.
// The predicates the four k_check_*_records kernels share, on the eight 32-bit words of a field -- compared as integers, not in the field:
// an amount below 2^128; an index inside the tree (u64 in the low bytes, < 2^depth, upper bytes zero); w <= a, most significant word first
__device__ __forceinline__ bool rec_amount_ok(const uint32_t* w) { return (w[4] | w[5] | w[6] | w[7]) == 0; }
__device__ __forceinline__ bool rec_index_ok(const uint32_t* w, int depth) {
  const uint64_t idx = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  return (w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0 && (depth >= 64 || (idx >> depth) == 0);
}
__device__ __forceinline__ bool rec_le(const uint32_t* w, const uint32_t* a) {
  bool gt = false, decided = false;
  for (int i = 7; i >= 0; i--) {
    if (!decided && w[i] != a[i]) { gt = w[i] > a[i]; decided = true; }
  }
  return !gt;
}

__global__ void __launch_bounds__(64) k_check_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(W_REC + depth)) return;
  const uint8_t* p = inputs + (g * (size_t)(W_REC + depth) + f) * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 5) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void withdraw_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_records, dim3(grid_for(W_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream, inputs_d, a.depth, n, bad_d);
}

// the descriptor's view of the shape (statements.h); the witness launches below keep their own
static RecordShape withdraw_record_shape(const StatementArgs& a) {
  const WithdrawShape s = withdraw_shape(a.depth, a.n_pad3, a.n_pad2);
  return RecordShape{s.n_wires, s.n_constraints, 0, s.first_gadget_wire, 0};
}

// ---- the walk on the HOST (round 6; opt-in: og_set_host_chains) ---------------------------------------------------------------------
// One request's Merkle walk is a chain of ~19 000 dependent Montgomery products (52 of its 72 permutations, k_withdraw_core_lat),
// and a chain runs at the latency of ONE product: ~900 shader cycles = 0.42 us on a lone wave -- a wave issues an instruction
// every ~4.8 cycles whatever it depends on, and the product is 205 of them (the wave-wide form of field_w9.hip.h
// takes 616 cycles and the k_w9_* kernels above walk with it: 7.4 -> 5.7 ms for one request -- the GPU's own best).
// A server core with 64-bit multipliers runs the same product -- the SAME code: the field layer is OG_HD, og_verify already runs
// it on the host -- in 20-50 ns.  So for calls of a handful of requests (the reference's handler proves ONE per HTTP call,
// /root/reference/src/services/api_services/withdraw.rs:27-71) the host may walk the chains: records down (1.3 KB each), one
// thread per request fills the core wires in Montgomery form exactly as k_withdraw_core<false> does, wire for wire, the
// wires go up (0.84 MB per request) and everything after -- the conversion, the padding gates, the sparse products, the quotient,
// the MSMs -- is the GPU's as before.  Not a fallback (the call still needs the GPU, and a batch never takes this path) and off
// by default: og_set_host_chains(ctx, max_requests) turns it on for calls of at most that many requests.  Same bytes as the
// kernels (tests/withdraw_cases.py, interpreter and GPU).
// one proof's core wires, k_withdraw_core<false> wire for wire (same gadget order, same wire indices), values in the host's form
static void withdraw_core_host(const H4* rc, const uint8_t* in, int depth, uint32_t first_gadget_wire, uint8_t* z) {
  const H4Field& f = h4_field();
  auto put = [&](uint32_t wire, const H4& v) { memcpy(z + (size_t)wire * 32, v.v, 32); };
  auto ld = [&](const uint8_t* p) { return h4_to_mont(f, h4_load(p)); };
  const H4 zero = {{0, 0, 0, 0}};
  const H4 nullifier = ld(in + W_NULLIFIER), secret = ld(in + W_SECRET), amount = ld(in + W_AMOUNT), recipient = ld(in + W_RECIPIENT);
  uint64_t index = 0;
  memcpy(&index, in + W_INDEX, 8);
  const H4 token = ld(in + W_TOKEN), chain_id = ld(in + W_CHAIN);
  put(0, f.one); put(3, recipient); put(4, amount); put(5, token); put(6, chain_id); put(7, nullifier); put(8, secret);
  for (int l = 0; l < depth; l++) {
    put(9 + l, ld(in + (size_t)(W_REC + l) * 32));
    put(9 + depth + l, ((index >> l) & 1) ? f.one : zero);
  }
  put(9 + 2 * depth, h4_mul(f, recipient, recipient));
  put(10 + 2 * depth, h4_mul(f, chain_id, chain_id));
  uint32_t w = first_gadget_wire;
  H4 cur = zero, inner = zero;
  for (int h = 0; h < 4 + depth; h++) {
    H4 l_in, r_in;
    int out_wire = -1;
    if (h == 0) { l_in = nullifier; r_in = secret; }
    else if (h == 1) { l_in = amount; r_in = token; }
    else if (h == 2) { l_in = inner; r_in = cur; }
    else if (h == 3) { l_in = nullifier; r_in = zero; out_wire = 2; }
    else {
      const int lvl = h - 4;
      const H4 sib = ld(in + (size_t)(W_REC + lvl) * 32);
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      put(w++, l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    }
    H4 k = zero, x = l_in, k1 = zero;
    for (int p = 0; p < 2; p++) {
      for (int i = 0; i < MIMC7_ROUNDS; i++) {
        const H4 t = h4_add(f, h4_add(f, x, k), rc[i]);
        const H4 t2 = h4_mul(f, t, t), t4 = h4_mul(f, t2, t2), t6 = h4_mul(f, t4, t2);
        x = h4_mul(f, t6, t);
        put(w, t2); put(w + 1, t4); put(w + 2, t6); put(w + 3, x);
        w += 4;
      }
      if (p == 0) {
        k1 = h4_add(f, l_in, x);
        put(w++, k1);
        k = k1;
        x = r_in;
      }
    }
    const H4 hout = h4_add(f, h4_add(f, h4_add(f, k1, k1), r_in), x);
    if (out_wire < 0) put(w++, hout); else put((uint32_t)out_wire, hout);
    if (h == 0) inner = hout;
    if (h != 3) cur = hout;
  }
}

// records (device) -> the core wires of n proofs in out_d (device, Montgomery form, as the core kernels leave them), via the host
static int withdraw_walk_on_host(og_ctx* ctx, int depth, const WithdrawShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  const size_t rec = (size_t)(W_REC + depth) * 32, core = (size_t)s.pad_base * 32, need = n * (rec + core);
  // the staging block is the context's: the upload of its previous user (another sub-batch of this call on the other lane, or a
  // submitted call still in flight) must have left it before the host writes into it again
  if (ctx->walk_ev) OG_HIP(hipEventSynchronize(ctx->walk_ev));
  else OG_HIP(hipEventCreateWithFlags(&ctx->walk_ev, hipEventDisableTiming));
  if (ctx->walk_stage_bytes < need) {
    if (ctx->walk_stage) (void)hipHostFree(ctx->walk_stage);
    ctx->walk_stage = nullptr;
    ctx->walk_stage_bytes = 0;
    OG_HIP(hipHostMalloc((void**)&ctx->walk_stage, need, 0));
    ctx->walk_stage_bytes = need;
  }
  uint8_t* recs = ctx->walk_stage + n * core;  // (the wires first: 16-byte aligned stores)
  OG_HIP(hipMemcpyAsync(recs, inputs_d, n * rec, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  const std::vector<H4> rc = h4_round_constants(ctx->mimc_consts_canon);  // (91 products: not worth a cache)
  const uint32_t fgw = (uint32_t)s.first_gadget_wire;
  auto walk = [&](size_t g) { withdraw_core_host(rc.data(), recs + g * rec, depth, fgw, ctx->walk_stage + g * core); };
  host_parallel_for(n, walk);  // a thread per request (a call that takes this path is a handful of requests)
  OG_HIP(hipMemcpy2DAsync(out_d, (size_t)s.n_wires * 32, ctx->walk_stage, core, core, n, hipMemcpyHostToDevice, ctx->stream));
  OG_HIP(hipEventRecord(ctx->walk_ev, ctx->stream));
  return OG_OK;
}

bool witness_walks_wave_wide(const og_ctx* ctx, size_t n) {
  return OG_HOOK_SET("OG_WITNESS_W9") ? OG_HOOK_INT("OG_WITNESS_W9", 1) != 0
                                      : std::max(n, ctx->call_requests) <= (size_t)OG_HOOK_INT("OG_WITNESS_W9_MAX", 512);
}

static int withdraw_witness(const Statement&, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  const int depth = a.depth;
  const uint64_t n_pad3 = a.n_pad3, n_pad2 = a.n_pad2;
  OG_REQUIRE(depth >= 1 && depth <= 64, "withdraw: depth must be 1..64");
  WithdrawShape s = withdraw_shape(depth, n_pad3, n_pad2);
  OG_REQUIRE(s.n_wires < (1ull << 31) && n_pad3 < (1ull << 30) && n_pad2 < (1ull << 30), "withdraw: too many wires");
  OG_REQUIRE(n <= 65535, "withdraw: at most 65535 witnesses per call");
  if (n == 0) return OG_OK;
  ProfScope ps(ctx, PROF_WITNESS, (double)n);
  // two lanes per proof (the latency-bound form) unless OG_MIMC_PAIR=0: a sub-batch is at most 256 proofs = 8 waves
  const bool pair = OG_HOOK_INT("OG_MIMC_PAIR", 1) != 0;  // (read per call: tests run both forms)
  // a handful of requests: a wave per proof, the independent permutations side by side (k_withdraw_core_lat); OG_WITNESS_LAT=0 | 1
  // forces either form, OG_WITNESS_LAT_MAX moves the bound (tests, A/B)
  const size_t lat_max = (size_t)OG_HOOK_INT("OG_WITNESS_LAT_MAX", 16);  // (64 requests: the two-lane form is level or better)
  const bool lat = OG_HOOK_SET("OG_WITNESS_LAT") ? OG_HOOK_INT("OG_WITNESS_LAT", 0) != 0 : (pair && n <= lat_max);
  const bool on_host = ctx->host_chains_max > 0 && std::max(n, ctx->call_requests) <= (size_t)ctx->host_chains_max;  // (a sub-batch of a larger call stays on the GPU)
  // the wave-wide form (k_w9_*): one permutation per wave in three launches (witness_walks_wave_wide: the rule every statement shares)
  // -- for calls of at most 512 requests: there the walk is on the call's critical path (measured, same box, natural statement:
  // witness 7.4 -> 5.7 ms for one request, 9.3 -> 5.8 for 8, 9.3 -> 6.4 for 64, 9.4 -> 6.9 for 512; the call 10.9 -> 8.7, 14.7 -> 11.1,
  // 26.5 -> 23.3, 115 -> 113 ms: profiles/r06k_ab_witness_w9.txt); a wave per PERMUTATION is ~19 x the wave-instructions of the
  // lane-pair form (nine useful lanes of 64), which a throughput batch would pay out of its accumulations
  const bool w9 = !on_host && witness_walks_wave_wide(ctx, n);
  if (w9) {
    uint32_t *wl = nullptr, *xch = nullptr;
    OG_TRY(arena_get(ctx, "wit.w9.limbs", n * (size_t)s.pad_base * 36, (void**)&wl));
    OG_TRY(arena_get(ctx, "wit.w9.xch", n * (size_t)(depth + W9_XCH) * 36, (void**)&xch));
    const uint32_t* c9 = (const uint32_t*)ctx->mimc_consts9_d;
    OG_W9_LAUNCH(k_w9_first, w9_rows(), dim3((unsigned)(n * (size_t)(3 + depth))), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.pad_base,
                       (uint32_t)s.first_gadget_wire, wl, xch);
    OG_W9_LAUNCH(k_w9_second, w9_rows(), dim3((unsigned)(n * 3)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.pad_base,
                       (uint32_t)s.first_gadget_wire, wl, xch);
    OG_W9_LAUNCH(k_w9_chain, w9_rows(), dim3((unsigned)n), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.pad_base,
                       (uint32_t)s.first_gadget_wire, wl, xch);
    OG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_wires_from_limbs, dim3(grid_for(s.pad_base, 256), (unsigned)n), dim3(256), 0, ctx->stream, (const uint32_t*)wl, out_d,
                       (size_t)s.n_wires, (uint32_t)s.pad_base);
    OG_HIP(hipGetLastError());
  } else if (on_host)
    OG_TRY(withdraw_walk_on_host(ctx, depth, s, inputs_d, n, out_d));
  else if (lat && depth <= WLAT_JOBS_A + WLAT_JOBS_B)
    hipLaunchKernelGGL(k_withdraw_core_lat, dim3((unsigned)n), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d, depth,
                       (size_t)s.n_wires, (uint32_t)s.first_gadget_wire, n, out_d);
  else if (pair)
    hipLaunchKernelGGL(k_withdraw_core<true>, dim3(grid_for(2 * n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d,
                     depth, (size_t)s.n_wires, (uint32_t)s.first_gadget_wire, n, out_d);
  else
    hipLaunchKernelGGL(k_withdraw_core<false>, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d,
                     depth, (size_t)s.n_wires, (uint32_t)s.first_gadget_wire, n, out_d);
  OG_HIP(hipGetLastError());
  if (!w9)
    hipLaunchKernelGGL(k_wires_from_mont, dim3(grid_for(s.pad_base, 256), (unsigned)n), dim3(256), 0, ctx->stream, out_d,
                       (size_t)s.n_wires, (uint32_t)s.pad_base, on_host ? 32u : 1u);
  OG_HIP(hipGetLastError());
  const uint64_t units = n_pad3 + (n_pad2 + PAD_SEGMENT - 1) / PAD_SEGMENT;
  if (units) {
    hipLaunchKernelGGL(k_withdraw_pad, dim3(grid_for(units, 256), (unsigned)n), dim3(256), 0, ctx->stream, inputs_d, depth,
                       (size_t)s.n_wires, (uint32_t)s.pad_base, (uint32_t)n_pad3, (uint32_t)n_pad2, out_d);
    OG_HIP(hipGetLastError());
  }
  return OG_OK;
}

// ---- the deposit statement (round 6; BASELINE.json north_star: "deposit/withdraw circuits") ----------------------------------------
// Spec: oracle/py/deposit.py.  public: commitment, depositor; private: nullifier, secret; commitment = H(nullifier, secret) -- ONE
// MultiMiMC7 gadget whose output is the public wire 1 -- and depositor bound by its square.  No reference counterpart: the
// snapshot's deposit (/root/reference/src/services/api_services/deposit.rs:32-154 -> /root/reference/src/blockchain/tx/mint_tx.rs:11-49)
// credits an account on the word of an L1 transaction hash and has no commitment at all.
// Input record per deposit, 3 x 32 B canonical LE: nullifier | secret | depositor.  Output: 735 wires x 32 B canonical:
//   0 one | 1 commitment | 2 depositor | 3 nullifier | 4 secret | 5 depositor^2 | 6.. perm0 (364) | k1 | perm1 (364)
constexpr int D_REC = 3, D_PUB = 2;
constexpr uint32_t D_WIRES = 6 + 729, D_CONSTRAINTS = 1 + 730;

// One lane per deposit (a batch is parallel across lanes; one request is two permutations = 0.33 ms of chain).  Montgomery
// values are stored and converted afterwards in parallel (k_wires_from_mont), as in k_withdraw_core.
__global__ void __launch_bounds__(64) k_deposit_witness(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs, size_t n,
                                                       uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)D_REC * 32;
  WireWriterT<false> ww{out + g * (size_t)D_WIRES * 32, 6};
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(in));
  const Fr secret = fe_to_mont(fe_load<FrParams>(in + 32));
  const Fr depositor = fe_to_mont(fe_load<FrParams>(in + 64));
  ww.put(0, Fr::one());
  ww.put(2, depositor);
  ww.put(3, nullifier);
  ww.put(4, secret);
  ww.put(5, fe_sqr(depositor));
  // MultiMiMC7([l, r], key 0): k1 = l + E_0(l); out = 2 k1 + r + E_k1(r), with E_k(x) = x_91 + k (one rolled body, no calls)
  Fr k = Fr::zero(), x = nullifier, k1 = Fr::zero();
#pragma unroll 1
  for (int p = 0; p < 2; p++) {
#pragma unroll 1
    for (int i = 0; i < MIMC7_ROUNDS; i++) {
      const Fr t = fe_add3_weak(x, k, mimc7_const(consts, i));
      const Fr t2 = fe_sqr(t);
      const Fr t4 = fe_sqr(t2);
      const Fr t6 = fe_mul(t4, t2);
      x = fe_mul(t6, t);
      ww.push(t2);
      ww.push(t4);
      ww.push(t6);
      ww.push(x);
    }
    if (p == 0) {
      k1 = fe_add(nullifier, x);
      ww.push(k1);
      k = k1;
      x = secret;
    }
  }
  ww.put(1, fe_add(fe_add(fe_dbl(k1), secret), x));
}

// bad[g] = lowest field of record g that is not the canonical encoding of an Fr element (0 nullifier, 1 secret, 2 depositor)
__global__ void __launch_bounds__(64) k_check_deposit_records(const uint8_t* __restrict__ inputs, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * D_REC) return;
  const size_t g = t / D_REC;
  const uint32_t f = (uint32_t)(t % D_REC);
  if (!fe_lt_modulus(fe_load<FrParams>(inputs + t * 32))) atomicMin(&bad[g], f);
}

static RecordShape deposit_shape(const StatementArgs&) { return RecordShape{D_WIRES, D_CONSTRAINTS, 0, 0, 0}; }

static void deposit_launch_check(og_ctx* ctx, const StatementArgs&, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_deposit_records, dim3(grid_for(n * D_REC, 64)), dim3(64), 0, ctx->stream, inputs_d, n, bad_d);
}

static int deposit_witness(const Statement&, og_ctx* ctx, const StatementArgs&, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  OG_REQUIRE(n <= 65535, "deposit: at most 65535 witnesses per call");
  if (n == 0) return OG_OK;
  ProfScope ps(ctx, PROF_WITNESS, (double)n);
  hipLaunchKernelGGL(k_deposit_witness, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d, n, out_d);
  OG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_wires_from_mont, dim3(grid_for(D_WIRES, 256), (unsigned)n), dim3(256), 0, ctx->stream, out_d, (size_t)D_WIRES, D_WIRES, 1u);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// The ONE rolled permutation body of the one-lane-per-request statement kernels (k_split_core, k_transfer_core): MultiMiMC7([l, r],
// key 0) with every wire of the gadget but its output pushed at the writer's cursor -- k1 = l + E_0(l); out = 2 k1 + r + E_k1(r), with
// E_k(x) = x_91 + k.  Inlined into the kernel's loop over gadgets (no device-function call).  Returns the gadget's output.
// (k_join_core keeps the same loop in its own text, with a store predicate per lane of its pairs: routed through here it compiles
// to one VGPR more, and the existing rows of the kernel-resource table stay what they are.)
__device__ __forceinline__ Fr gadget_wires(const uint32_t* __restrict__ consts, WireWriterT<false>& ww, const Fr& l_in, const Fr& r_in) {
  Fr k = Fr::zero(), x = l_in, k1 = Fr::zero();
#pragma unroll 1
  for (int p = 0; p < 2; p++) {
#pragma unroll 1
    for (int i = 0; i < MIMC7_ROUNDS; i++) {
      const Fr t = fe_add3_weak(x, k, mimc7_const(consts, i));  // < 5N, only ever multiplied
      const Fr t2 = fe_sqr(t);
      const Fr t4 = fe_sqr(t2);
      const Fr t6 = fe_mul(t4, t2);
      x = fe_mul(t6, t);
      ww.push(t2);
      ww.push(t4);
      ww.push(t6);
      ww.push(x);
    }
    if (p == 0) {
      k1 = fe_add(l_in, x);
      ww.push(k1);
      k = k1;
      x = r_in;
    }
  }
  return fe_add(fe_add(fe_dbl(k1), r_in), x);
}

// ---- the split statement: withdraw part of a note, keep the rest as a change note ---------------------------------------------------
// Spec: tests/split_spec.py.  public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf (n_pub = 7); private:
// nullifier, secret, amount, change_commitment, change, the path.  The note leaf = H(H(nullifier, secret), H(amount, token)) lies under
// root, nullifier_hash = H(nullifier, 0), amount_out + change = amount with both below 2^128 (a 128-bit decomposition each: the sum
// cannot wrap, which is what stops an overdraw), change_leaf = H(change_commitment, H(change, token)) -- a leaf of the deposit
// shape, which og_mimc7_append_d appends.  `amount` is private here.  No reference counterpart (the snapshot's withdraw is a whole-
// amount ECDSA-authorised burn, /root/reference/src/services/api_services/withdraw.rs:27-71).
// Input record per request, (9 + depth) x 32 B canonical LE:
//   nullifier | secret | amount | recipient | amount_out | index (u64 in the low bytes) | token | chain_id | change_commitment | siblings[depth]
// Wires:
//   0 one | 1 root | 2 nullifier_hash | 3 recipient | 4 amount_out | 5 token | 6 chain_id | 7 change_leaf
//   8 nullifier | 9 secret | 10 amount | 11 change_commitment | 12 change | 13.. siblings[D] | index bits[D] | recipient^2 | chain_id^2
//   | amount_out bits[128] (LSB first) | change bits[128] | the gadgets: inner, asset, leaf, nullifier_hash (out = wire 2), level
//   0..D-1 (the last one's out = wire 1), change_asset = H(change, token), change_leaf = H(change_commitment, change_asset) (out = wire 7)
// Two walks: k_split_core (one lane per request, the form for batches) and k_sw9_* (a permutation per wave in three launches, for
// calls of at most 512 requests: at the end of the file).  NOT built for this statement: the t^4 | t^3 lane-pair round, the
// wave-per-request walk, host chains.
constexpr int S_PUB = 7;
constexpr int S_REC = 9;  // fields of a split record before the siblings
constexpr int S_BITS = 128;
// byte offsets of the record's fields
constexpr int S_NULLIFIER = 0, S_SECRET = 32, S_AMOUNT = 64, S_RECIPIENT = 96, S_AMOUNT_OUT = 128, S_INDEX = 160, S_TOKEN = 192, S_CHAIN = 224,
              S_CHANGE_COMMITMENT = 256;

static RecordShape split_shape(const StatementArgs& a) {
  RecordShape s{};
  const int depth = a.depth;
  const uint64_t hashes = 6 + (uint64_t)depth;
  s.first_bit_wire = 1 + S_PUB + 5 + 2 * (uint64_t)depth + 2;
  s.first_gadget_wire = s.first_bit_wire + 2 * S_BITS;
  s.n_wires = s.first_bit_wire + 2 * S_BITS + depth + hashes * 730 - 3;  // (the gadgets follow the bit wires)
  s.n_constraints = 3 + 2 * (S_BITS + 1) + 2 * (uint64_t)depth + hashes * 730;
  return s;
}

// One lane per request, as k_withdraw_core<false>: the (6 + depth) MultiMiMC7 gadgets run through ONE inlined permutation body (rolled
// loops over gadgets, the two permutations of a gadget, and the 91 rounds), no device-function calls; Montgomery values are stored
// and k_wires_from_mont converts them afterwards, in parallel.  `change` and the 256 bit wires come from the record's integer words
// (the records are checked first: amount_out <= amount < 2^128, so the difference does not borrow).
__global__ void __launch_bounds__(64) k_split_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs, int depth,
                                                  size_t n_wires, uint32_t first_bit_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(S_REC + depth) * 32;
  WireWriterT<false> ww{out + g * n_wires * 32, first_bit_wire};
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(in + S_NULLIFIER));
  const Fr secret = fe_to_mont(fe_load<FrParams>(in + S_SECRET));
  const Fr amount = fe_to_mont(fe_load<FrParams>(in + S_AMOUNT));
  const Fr recipient = fe_to_mont(fe_load<FrParams>(in + S_RECIPIENT));
  const Fr amount_out = fe_to_mont(fe_load<FrParams>(in + S_AMOUNT_OUT));
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + S_INDEX);
  const Fr token = fe_to_mont(fe_load<FrParams>(in + S_TOKEN));
  const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + S_CHAIN));
  const Fr change_commitment = fe_to_mont(fe_load<FrParams>(in + S_CHANGE_COMMITMENT));
  // change = amount - amount_out on the integer words
  const uint64_t a_lo = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT), a_hi = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT + 8);
  const uint64_t o_lo = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT_OUT), o_hi = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT_OUT + 8);
  const uint64_t c_lo = a_lo - o_lo, c_hi = a_hi - o_hi - (a_lo < o_lo ? 1u : 0u);
  const uint32_t cw[8] = {(uint32_t)c_lo, (uint32_t)(c_lo >> 32), (uint32_t)c_hi, (uint32_t)(c_hi >> 32), 0u, 0u, 0u, 0u};
  const Fr change = fe_to_mont(fe_from_words<FrParams>(cw));
  ww.put(0, Fr::one());
  ww.put(3, recipient);
  ww.put(4, amount_out);
  ww.put(5, token);
  ww.put(6, chain_id);
  ww.put(8, nullifier);
  ww.put(9, secret);
  ww.put(10, amount);
  ww.put(11, change_commitment);
  ww.put(12, change);
  for (int l = 0; l < depth; l++) {
    ww.put(13 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(S_REC + l) * 32)));
    ww.put(13 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  ww.put(13 + 2 * depth, fe_sqr(recipient));
  ww.put(14 + 2 * depth, fe_sqr(chain_id));
#pragma unroll 1
  for (int v = 0; v < 2; v++) {  // the bits of amount_out, then of change, LSB first
    const uint64_t lo = v ? c_lo : o_lo, hi = v ? c_hi : o_hi;
#pragma unroll 1
    for (int i = 0; i < S_BITS; i++) ww.push((((i < 64 ? lo : hi) >> (i & 63)) & 1) ? Fr::one() : Fr::zero());
  }
  // gadget 0: inner = H(nullifier, secret); 1: asset = H(amount, token); 2: leaf = H(inner, asset); 3: nullifier_hash =
  // H(nullifier, 0) -> wire 2; 4 + l: level l of the path (wire 1 = root for the last level); 4 + depth: change_asset =
  // H(change, token); 5 + depth: change_leaf = H(change_commitment, change_asset) -> wire 7
  Fr cur = Fr::zero(), inner = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 6 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = nullifier; r_in = secret;
    } else if (h == 1) {
      l_in = amount; r_in = token;
    } else if (h == 2) {
      l_in = inner; r_in = cur;
    } else if (h == 3) {
      l_in = nullifier; r_in = Fr::zero(); out_wire = 2;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = fe_to_mont(fe_load<FrParams>(in + (size_t)(S_REC + lvl) * 32));
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    } else if (h == 4 + depth) {
      l_in = change; r_in = token;
    } else {
      l_in = change_commitment; r_in = cur; out_wire = 7;
    }
    const Fr hout = gadget_wires(consts, ww, l_in, r_in);
    if (out_wire < 0) ww.push(hout); else ww.put((uint32_t)out_wire, hout);
    if (h == 0) inner = hout;
    if (h != 3) cur = hout;
  }
}

// Boundary check of the split records, one lane per field as k_check_records: every field canonical (< r), the index inside the
// tree, amount < 2^128 (field 2), amount_out < 2^128 and amount_out <= amount (field 4) -- compared on the integer words, not in the
// field.  bad[g] = lowest offending field of record g (the caller initialises it to 0xffffffff): 0 nullifier, 1 secret, 2 amount,
// 3 recipient, 4 amount_out, 5 index, 6 token, 7 chain_id, 8 change_commitment, 9 + l sibling l.
__global__ void __launch_bounds__(64) k_check_split_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(S_REC + depth)) return;
  const uint8_t* rec = inputs + g * (size_t)(S_REC + depth) * 32;
  const uint8_t* p = rec + (size_t)f * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 2 || f == 4) ok = ok && rec_amount_ok(w);
  if (f == 4) ok = ok && rec_le(w, reinterpret_cast<const uint32_t*>(rec + S_AMOUNT));  // amount_out <= amount
  if (f == 5) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void split_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_split_records, dim3(grid_for(S_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream, inputs_d, a.depth, n, bad_d);
}

static void split_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_split_core, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d, depth,
                     (size_t)s.n_wires, (uint32_t)s.first_bit_wire, n, out_d);
}

// ---- the join statement: merge two notes into one -----------------------------------------------------------------------------------
// Spec: tests/join_spec.py.  public: root, nullifier_hash_a, nullifier_hash_b, chain_id, out_leaf (n_pub = 5); private: per note
// nullifier, secret, amount and a path; token (ONE wire for all three asset hashes: nothing is paid out), out_commitment, sum,
// nh_diff_inv.  For x in {a, b}: leaf_x = H(H(nullifier_x, secret_x), H(amount_x, token)) lies under root at index_x and
// nullifier_hash_x = H(nullifier_x, 0); the last level of BOTH walks has wire 1 as its output wire, which is what says "the same
// root"; amount_a + amount_b = sum with all three below 2^128 (a 128-bit decomposition each); (nullifier_hash_a - nullifier_hash_b)
// nh_diff_inv = 1, so the same note cannot be counted twice; out_leaf = H(out_commitment, H(sum, token)), a leaf of the deposit shape,
// which og_mimc7_append_d appends.  No reference counterpart (the snapshot has no circuit).
// Input record per request, (11 + 2 depth) x 32 B canonical LE:
//   nullifier_a | secret_a | amount_a | index_a (u64 in the low bytes) | nullifier_b | secret_b | amount_b | index_b | token | chain_id
//   | out_commitment | siblings_a[depth] | siblings_b[depth]
// Wires:
//   0 one | 1 root | 2 nullifier_hash_a | 3 nullifier_hash_b | 4 chain_id | 5 out_leaf
//   6 nullifier_a | 7 secret_a | 8 amount_a | 9 nullifier_b | 10 secret_b | 11 amount_b | 12 token | 13 out_commitment | 14 sum
//   | 15 nh_diff_inv | 16.. siblings_a[D] | siblings_b[D] | index bits a[D] | index bits b[D] | chain_id^2 | amount_a bits[128] (LSB
//   first) | amount_b bits[128] | sum bits[128] | the gadgets of note a: inner, asset, leaf, nullifier_hash (out = wire 2), level
//   0..D-1 (the last one's out = wire 1) | the same gadgets of note b (outs = wire 3 and wire 1) | out_asset = H(sum, token),
//   out_leaf = H(out_commitment, out_asset) (out = wire 5)
// Two walks: k_join_core (two lanes per request, the form for batches) and k_jw9_* (a permutation per wave in three launches, for
// calls of at most 512 requests: at the end of the file).  NOT built for this statement (as for split): the t^4 | t^3 lane-pair
// round, the wave-per-request walk, host chains.
constexpr int J_PUB = 5;
constexpr int J_REC = 11;  // fields of a join record before the siblings
constexpr int J_BITS = 128;

static RecordShape join_shape(const StatementArgs& a) {
  RecordShape s{};
  const int depth = a.depth;
  const uint64_t hashes = 10 + 2 * (uint64_t)depth;
  s.first_bit_wire = 1 + J_PUB + 10 + 4 * (uint64_t)depth + 1;
  s.first_gadget_wire = s.first_bit_wire + 3 * J_BITS;
  s.note_gadget_wires = (4 + (uint64_t)depth) * 730 + depth - 2;  // a `left` per level; nullifier_hash and root are public wires
  s.n_wires = s.first_bit_wire + 3 * J_BITS + 2 * s.note_gadget_wires + 2 * 730 - 1;
  s.n_constraints = 3 + 3 * (J_BITS + 1) + 4 * (uint64_t)depth + hashes * 730;
  return s;
}

// TWO lanes per request: lane 2g walks note a, lane 2g + 1 note b, through the ONE rolled permutation body of k_split_core -- the same
// instruction stream, uniform trip counts, no device-function calls -- so the two walks cost the wave what one costs and the
// dependent chain is 6 + depth gadgets deep (4 + depth of a walk, then the two output gadgets) instead of 10 + 2 depth.  Each lane
// stores its own note's input wires and gadget wires at its own cursor; the even lane alone stores the public and shared wires,
// chain_id^2, the 384 bit wires (from the record's integer words: the records are checked first, amount_a + amount_b < 2^128), wire 1
// from note a's walk, the two output gadgets (the odd lane runs them beside it on its own values and stores nothing) and
// nh_diff_inv, for which it gets nullifier_hash_b from its neighbour (pair_swap) -- one fe_inv, ~380 products behind a chain of
// ~27 000, not worth spreading.  Every wire is stored by exactly one lane, as a Montgomery value; k_wires_from_mont converts afterwards.
// A pair never straddles a wave or the end of the batch: both lanes of a pair leave together.
__global__ void __launch_bounds__(64) k_join_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs, int depth,
                                                 size_t n_wires, uint32_t first_bit_wire, uint32_t note_gadget_wires, size_t n,
                                                 uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x, g = lane >> 1;
  if (g >= n) return;
  const bool odd = threadIdx.x & 1, even = !odd;
  const uint32_t b = odd ? 1u : 0u;
  const uint8_t* in = inputs + g * (size_t)(J_REC + 2 * depth) * 32;
  const uint8_t* note = in + (size_t)b * 128;                               // nullifier | secret | amount | index of this lane's note
  const uint8_t* sibs = in + (size_t)(J_REC + b * (uint32_t)depth) * 32;    // its siblings
  const uint32_t first_gadget_wire = first_bit_wire + 3 * J_BITS;
  WireWriterT<false> ww{out + g * n_wires * 32, first_gadget_wire + b * note_gadget_wires};
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(note));
  const Fr secret = fe_to_mont(fe_load<FrParams>(note + 32));
  const Fr amount = fe_to_mont(fe_load<FrParams>(note + 64));
  const uint64_t index = *reinterpret_cast<const uint64_t*>(note + 96);
  const Fr token = fe_to_mont(fe_load<FrParams>(in + 256));
  const Fr out_commitment = fe_to_mont(fe_load<FrParams>(in + 320));
  // sum = amount_a + amount_b on the integer words
  const uint64_t a_lo = *reinterpret_cast<const uint64_t*>(in + 64), a_hi = *reinterpret_cast<const uint64_t*>(in + 72);
  const uint64_t b_lo = *reinterpret_cast<const uint64_t*>(in + 192), b_hi = *reinterpret_cast<const uint64_t*>(in + 200);
  const uint64_t s_lo = a_lo + b_lo, s_hi = a_hi + b_hi + (s_lo < a_lo ? 1u : 0u);
  const uint32_t sw[8] = {(uint32_t)s_lo, (uint32_t)(s_lo >> 32), (uint32_t)s_hi, (uint32_t)(s_hi >> 32), 0u, 0u, 0u, 0u};
  const Fr sum = fe_to_mont(fe_from_words<FrParams>(sw));
  ww.put(6 + 3 * b, nullifier);
  ww.put(7 + 3 * b, secret);
  ww.put(8 + 3 * b, amount);
  for (int l = 0; l < depth; l++) {
    ww.put(16 + b * (uint32_t)depth + l, fe_to_mont(fe_load<FrParams>(sibs + (size_t)l * 32)));
    ww.put(16 + (2 + b) * (uint32_t)depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  if (even) {
    const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + 288));
    ww.put(0, Fr::one());
    ww.put(4, chain_id);
    ww.put(12, token);
    ww.put(13, out_commitment);
    ww.put(14, sum);
    ww.put(16 + 4 * depth, fe_sqr(chain_id));
    uint32_t w = first_bit_wire;
#pragma unroll 1
    for (int v = 0; v < 3; v++) {  // the bits of amount_a, amount_b, sum, LSB first
      const uint64_t lo = v == 0 ? a_lo : v == 1 ? b_lo : s_lo, hi = v == 0 ? a_hi : v == 1 ? b_hi : s_hi;
#pragma unroll 1
      for (int i = 0; i < J_BITS; i++) ww.put(w++, (((i < 64 ? lo : hi) >> (i & 63)) & 1) ? Fr::one() : Fr::zero());
    }
  }
  // gadget 0: inner = H(nullifier, secret); 1: asset = H(amount, token); 2: leaf = H(inner, asset); 3: nullifier_hash =
  // H(nullifier, 0) -> wire 2 | 3; 4 + l: level l of this lane's path (the last one's output is the root: wire 1, stored by the even
  // lane); then, stored by the even lane alone, 4 + depth: out_asset = H(sum, token); 5 + depth: out_leaf = H(out_commitment,
  // out_asset) -> wire 5
  Fr cur = Fr::zero(), inner = Fr::zero(), nh = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 6 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    bool mine = true, mine_out = true;  // does this lane store the gadget's wires / its output
    if (h == 0) {
      l_in = nullifier; r_in = secret;
    } else if (h == 1) {
      l_in = amount; r_in = token;
    } else if (h == 2) {
      l_in = inner; r_in = cur;
    } else if (h == 3) {
      l_in = nullifier; r_in = Fr::zero(); out_wire = 2 + (int)b;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = fe_to_mont(fe_load<FrParams>(sibs + (size_t)lvl * 32));
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) { out_wire = 1; mine_out = even; }
    } else if (h == 4 + depth) {
      l_in = sum; r_in = token; mine = mine_out = even;
      ww.w = first_gadget_wire + 2 * note_gadget_wires;
    } else {
      l_in = out_commitment; r_in = cur; out_wire = 5; mine = mine_out = even;
    }
    // MultiMiMC7([l, r], key 0): k1 = l + E_0(l); out = 2 k1 + r + E_k1(r), with E_k(x) = x_91 + k
    Fr k = Fr::zero(), x = l_in, k1 = Fr::zero();
#pragma unroll 1
    for (int p = 0; p < 2; p++) {
#pragma unroll 1
      for (int i = 0; i < MIMC7_ROUNDS; i++) {
        const Fr t = fe_add3_weak(x, k, mimc7_const(consts, i));  // < 5N, only ever multiplied
        const Fr t2 = fe_sqr(t);
        const Fr t4 = fe_sqr(t2);
        const Fr t6 = fe_mul(t4, t2);
        x = fe_mul(t6, t);
        ww.push_if(mine, t2);
        ww.push_if(mine, t4);
        ww.push_if(mine, t6);
        ww.push_if(mine, x);
      }
      if (p == 0) {
        k1 = fe_add(l_in, x);
        ww.push_if(mine, k1);
        k = k1;
        x = r_in;
      }
    }
    const Fr hout = fe_add(fe_add(fe_dbl(k1), r_in), x);
    if (out_wire < 0) ww.push_if(mine_out, hout); else ww.put_if(mine_out, (uint32_t)out_wire, hout);
    if (h == 0) inner = hout;
    if (h == 3) nh = hout; else cur = hout;
  }
  // nh_diff_inv = 1 / (nullifier_hash_a - nullifier_hash_b): both lanes of the pair are here (the swap needs them); the operands are
  // SELECTED so that both lanes form a - b, never b - a, and the even one stores
  const Fr nh_other = pair_swap(nh);
  const Fr inv = fe_inv(fe_sub(pair_select(odd, nh_other, nh), pair_select(odd, nh, nh_other)));
  ww.put_if(even, 15, inv);
}

// Boundary check of the join records, one lane per field as k_check_split_records: every field canonical (< r), both indices inside
// the tree (fields 3, 7), amount_a < 2^128 (field 2), amount_b < 2^128 and amount_a + amount_b < 2^128 (field 6) -- compared on the
// integer words, not in the field --, and nullifier_b != nullifier_a (field 4: nh_diff_inv would not exist).  bad[g] = lowest
// offending field of record g (the caller initialises it to 0xffffffff): 0 nullifier_a, 1 secret_a, 2 amount_a, 3 index_a,
// 4 nullifier_b, 5 secret_b, 6 amount_b, 7 index_b, 8 token, 9 chain_id, 10 out_commitment, 11 + l sibling a of level l,
// 11 + depth + l sibling b of level l.
__global__ void __launch_bounds__(64) k_check_join_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(J_REC + 2 * depth)) return;
  const uint8_t* rec = inputs + g * (size_t)(J_REC + 2 * depth) * 32;
  const uint8_t* p = rec + (size_t)f * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 2 || f == 6) ok = ok && rec_amount_ok(w);
  if (f == 6) {  // amount_a + amount_b < 2^128 as integers: no carry into word 4 or out of word 7
    const uint32_t* a = reinterpret_cast<const uint32_t*>(rec + 64);
    uint64_t carry = 0;
    uint32_t high = 0;
    for (int i = 0; i < 8; i++) {
      carry += (uint64_t)a[i] + w[i];
      if (i >= 4) high |= (uint32_t)carry;
      carry >>= 32;
    }
    ok = ok && high == 0 && carry == 0;
  }
  if (f == 4) {  // nullifier_b != nullifier_a
    const uint32_t* a = reinterpret_cast<const uint32_t*>(rec);
    uint32_t diff = 0;
    for (int i = 0; i < 8; i++) diff |= a[i] ^ w[i];
    ok = ok && diff != 0;
  }
  if (f == 3 || f == 7) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void join_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_join_records, dim3(grid_for(J_REC + 2 * a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream, inputs_d, a.depth, n, bad_d);
}

static void join_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_join_core, dim3(grid_for(2 * n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d, depth,
                     (size_t)s.n_wires, (uint32_t)s.first_bit_wire, (uint32_t)s.note_gadget_wires, n, out_d);
}

// ---- the transfer statement: pay part of a note inside the pool, keep the rest ------------------------------------------------------
// Spec: tests/transfer_spec.py.  public: root, nullifier_hash, chain_id, pay_leaf, change_leaf (n_pub = 5); private: nullifier, secret,
// amount, token (ONE wire for all three asset hashes, private as in join: nothing is paid out), pay_commitment, pay_amount,
// change_commitment, change, the path.  The note leaf = H(H(nullifier, secret), H(amount, token)) lies under root, nullifier_hash =
// H(nullifier, 0), pay_amount + change = amount with both below 2^128 (a 128-bit decomposition each: the sum cannot wrap, which is what
// makes it impossible to create value), pay_leaf = H(pay_commitment, H(pay_amount, token)) and change_leaf = H(change_commitment,
// H(change, token)) -- two leaves of the deposit shape, which og_mimc7_append_d appends in that order.  Nothing leaves the pool.  No
// reference counterpart (the snapshot has no circuit).
// Input record per request, (9 + depth) x 32 B canonical LE:
//   nullifier | secret | amount | index (u64 in the low bytes) | token | chain_id | pay_commitment | pay_amount | change_commitment | siblings[depth]
// Wires:
//   0 one | 1 root | 2 nullifier_hash | 3 chain_id | 4 pay_leaf | 5 change_leaf
//   6 nullifier | 7 secret | 8 amount | 9 token | 10 pay_commitment | 11 pay_amount | 12 change_commitment | 13 change
//   14.. siblings[D] | index bits[D] | chain_id^2 | pay_amount bits[128] (LSB first) | change bits[128] | the gadgets: inner, asset, leaf,
//   nullifier_hash (out = wire 2), level 0..D-1 (the last one's out = wire 1), pay_asset = H(pay_amount, token), pay_leaf =
//   H(pay_commitment, pay_asset) (out = wire 4), change_asset = H(change, token), change_leaf = H(change_commitment, change_asset) (out = wire 5)
// Two walks: k_transfer_core (one lane per request, the form for batches) and k_tw9_* (a permutation per wave in three launches, for
// calls of at most 512 requests: the rule of withdraw's k_w9_*).  NOT built for this statement: the t^4 | t^3 lane-pair round, the
// wave-per-request walk, host chains.
constexpr int T_PUB = 5;
constexpr int T_REC = 9;  // fields of a transfer record before the siblings
constexpr int T_BITS = 128;
// byte offsets of the record's fields
constexpr int T_NULLIFIER = 0, T_SECRET = 32, T_AMOUNT = 64, T_INDEX = 96, T_TOKEN = 128, T_CHAIN = 160, T_PAY_COMMITMENT = 192, T_PAY_AMOUNT = 224,
              T_CHANGE_COMMITMENT = 256;

static RecordShape transfer_shape(const StatementArgs& a) {
  RecordShape s{};
  const int depth = a.depth;
  const uint64_t hashes = 8 + (uint64_t)depth;
  s.first_bit_wire = 1 + T_PUB + 8 + 2 * (uint64_t)depth + 1;
  s.first_gadget_wire = s.first_bit_wire + 2 * T_BITS;
  s.n_wires = s.first_gadget_wire + depth + hashes * 730 - 4;  // a `left` per level; nullifier_hash, root and the two leaves are public wires
  s.n_constraints = 2 + 2 * (T_BITS + 1) + 2 * (uint64_t)depth + hashes * 730;
  return s;
}

// change = amount - pay_amount on the record's integer words (the records are checked first: pay_amount <= amount < 2^128, so the
// difference does not borrow): its two 64-bit halves, and the field element
struct TransferChange {
  uint64_t p_lo, p_hi, c_lo, c_hi;
  __device__ __forceinline__ Fr value() const {
    const uint32_t cw[8] = {(uint32_t)c_lo, (uint32_t)(c_lo >> 32), (uint32_t)c_hi, (uint32_t)(c_hi >> 32), 0u, 0u, 0u, 0u};
    return fe_to_mont(fe_from_words<FrParams>(cw));
  }
};
__device__ __forceinline__ TransferChange transfer_change(const uint8_t* in) {
  const uint64_t a_lo = *reinterpret_cast<const uint64_t*>(in + T_AMOUNT), a_hi = *reinterpret_cast<const uint64_t*>(in + T_AMOUNT + 8);
  TransferChange c;
  c.p_lo = *reinterpret_cast<const uint64_t*>(in + T_PAY_AMOUNT);
  c.p_hi = *reinterpret_cast<const uint64_t*>(in + T_PAY_AMOUNT + 8);
  c.c_lo = a_lo - c.p_lo;
  c.c_hi = a_hi - c.p_hi - (a_lo < c.p_lo ? 1u : 0u);
  return c;
}
// bit i (0 .. 255) of pay_amount | change, as a wire
__device__ __forceinline__ Fr transfer_bit_wire(const TransferChange& c, int i) {
  const uint64_t word = i < 64 ? c.p_lo : i < 128 ? c.p_hi : i < 192 ? c.c_lo : c.c_hi;
  return ((word >> (i & 63)) & 1) ? Fr::one() : Fr::zero();
}

// One lane per request, as k_split_core: the (8 + depth) MultiMiMC7 gadgets through the one rolled permutation body (gadget_wires), no
// device-function calls; Montgomery values are stored and k_wires_from_mont converts them afterwards, in parallel.
__global__ void __launch_bounds__(64) k_transfer_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ inputs, int depth,
                                                     size_t n_wires, uint32_t first_bit_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(T_REC + depth) * 32;
  WireWriterT<false> ww{out + g * n_wires * 32, first_bit_wire};
  const Fr nullifier = fe_to_mont(fe_load<FrParams>(in + T_NULLIFIER));
  const Fr secret = fe_to_mont(fe_load<FrParams>(in + T_SECRET));
  const Fr amount = fe_to_mont(fe_load<FrParams>(in + T_AMOUNT));
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + T_INDEX);
  const Fr token = fe_to_mont(fe_load<FrParams>(in + T_TOKEN));
  const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + T_CHAIN));
  const Fr pay_commitment = fe_to_mont(fe_load<FrParams>(in + T_PAY_COMMITMENT));
  const Fr pay_amount = fe_to_mont(fe_load<FrParams>(in + T_PAY_AMOUNT));
  const Fr change_commitment = fe_to_mont(fe_load<FrParams>(in + T_CHANGE_COMMITMENT));
  const TransferChange chg = transfer_change(in);
  const Fr change = chg.value();
  ww.put(0, Fr::one());
  ww.put(3, chain_id);
  ww.put(6, nullifier);
  ww.put(7, secret);
  ww.put(8, amount);
  ww.put(9, token);
  ww.put(10, pay_commitment);
  ww.put(11, pay_amount);
  ww.put(12, change_commitment);
  ww.put(13, change);
  for (int l = 0; l < depth; l++) {
    ww.put(14 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(T_REC + l) * 32)));
    ww.put(14 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  ww.put(14 + 2 * depth, fe_sqr(chain_id));
#pragma unroll 1
  for (int i = 0; i < 2 * T_BITS; i++) ww.push(transfer_bit_wire(chg, i));  // the bits of pay_amount, then of change, LSB first
  // gadget 0: inner = H(nullifier, secret); 1: asset = H(amount, token); 2: leaf = H(inner, asset); 3: nullifier_hash =
  // H(nullifier, 0) -> wire 2; 4 + l: level l of the path (wire 1 = root for the last level); 4 + depth: pay_asset = H(pay_amount,
  // token); 5 + depth: pay_leaf = H(pay_commitment, pay_asset) -> wire 4; 6 + depth: change_asset = H(change, token); 7 + depth:
  // change_leaf = H(change_commitment, change_asset) -> wire 5
  Fr cur = Fr::zero(), inner = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 8 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = nullifier; r_in = secret;
    } else if (h == 1) {
      l_in = amount; r_in = token;
    } else if (h == 2) {
      l_in = inner; r_in = cur;
    } else if (h == 3) {
      l_in = nullifier; r_in = Fr::zero(); out_wire = 2;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = fe_to_mont(fe_load<FrParams>(in + (size_t)(T_REC + lvl) * 32));
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    } else if (h == 4 + depth) {
      l_in = pay_amount; r_in = token;
    } else if (h == 5 + depth) {
      l_in = pay_commitment; r_in = cur; out_wire = 4;
    } else if (h == 6 + depth) {
      l_in = change; r_in = token;
    } else {
      l_in = change_commitment; r_in = cur; out_wire = 5;
    }
    const Fr hout = gadget_wires(consts, ww, l_in, r_in);
    if (out_wire < 0) ww.push(hout); else ww.put((uint32_t)out_wire, hout);
    if (h == 0) inner = hout;
    if (h != 3) cur = hout;
  }
}

// The wave-wide form of the same walk (the header of k_w9_*: ONE permutation per one-wave workgroup, values between the launches as
// nine lazy limbs in xch, wires as nine limbs in wl for k_wires_from_limbs, the bounds of mimc7.hip.h w9_mimc7_round -- every hash
// output passes the strict product by one, w9_renorm, before it is anybody's input).  The two output notes do not depend on the
// Merkle walk, so all eight of their permutations sit BESIDE the dependent chain, which is exactly as long as withdraw's:
//   k_tw9_first   grid n x (7 + depth): E_0 of nullifier (wires of gadgets 0 and 3), amount, pay_amount, change, pay_commitment and
//                 change_commitment; E_0(sibling_l) of every level whose path node is the RIGHT input; one workgroup for the wires
//                 that are inputs, the square, the index bits and the 256 bit wires
//   k_tw9_second  grid n x 5: the second permutations of inner, asset, nullifier_hash, pay_asset, change_asset
//   k_tw9_chain   grid n x 3: block 0 is the chain (leaf, then the levels: k_w9_chain's work); blocks 1 and 2 are the second
//                 permutations of pay_leaf and change_leaf
// xch slots per request beyond the levels: [depth + 0] k1 of inner / nullifier_hash, [1] k1 of asset, [2] inner, [3] asset, [4] k1 of
// pay_asset, [5] k1 of change_asset, [6] k1 of pay_leaf, [7] k1 of change_leaf, [8] pay_asset, [9] change_asset, [10 .. 13]: 36 words
// nobody reads -- where the lanes without a limb store (w9_permute `dump`)
constexpr int TW9_XCH = 14, TW9_DUMP = 10;
// first wire of gadget h (for a level: of its hash, behind the `left` wire)
__device__ __forceinline__ uint32_t tw9_gadget_base(uint32_t fgw, int depth, int h) {
  if (h < 4) return fgw + (uint32_t)h * 730u;
  if (h < 4 + depth) return w9_gadget_base(fgw, h) + 1u;
  const uint32_t ob = fgw + 2918u + 731u * (uint32_t)depth;  // behind the levels (the last one's output is wire 1)
  return ob + (h == 4 + depth ? 0u : h == 5 + depth ? 730u : h == 6 + depth ? 1459u : 2189u);  // (pay_leaf's output is wire 4)
}
// the rest of H(l, r) once k1 = l + E_0(l) is there: the second permutation's wires behind k1's, the output (below 2 N) at out_wire
template <int FORM>
__device__ __forceinline__ uint32_t tw9_second_half(const uint32_t* __restrict__ consts9, uint32_t r_in, uint32_t k1, uint32_t nj, int tid, int lane,
                                                    uint32_t* __restrict__ wl, uint32_t base, uint32_t out_wire, uint32_t* __restrict__ dump) {
  const uint32_t xr = w9_permute<FORM, false>(consts9, r_in, k1, nj, tid, lane, wl, base + 365, 0u, dump);
  const uint32_t h = w9_renorm(2u * k1 + r_in + xr, nj, lane);
  w9_store(wl, out_wire, h, tid);
  return h;
}

// The chain block of split and of join (k_sw9_chain, k_jw9_chain: further down), k_tw9_chain's walk with the record and the note as
// parameters: leaf = H(inner, asset) (xch slots vals[0], vals[1]), then per level two permutations (the path node is the left input)
// or one (right: E_0(sibling), k1 and the selector wire came from the first launch, xch slot lvls[l]).  `fgw` is the first gadget
// wire of the note, `sibs` its siblings.  root = false (join's note b): the last level's output is nobody's wire -- wire 1 is note
// a's -- so its second permutation leaves its round wires and nothing else.  (k_tw9_chain keeps its own text: through here it
// compiles to 41 VGPRs instead of 43, and the existing rows of the kernel-resource table stay what they are.)
template <int FORM>
__device__ __forceinline__ void w9_note_chain(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ sibs, uint64_t index, int depth,
                                              uint32_t fgw, bool root, uint32_t* __restrict__ wl, const uint32_t* lvls, const uint32_t* vals,
                                              uint32_t* dump, uint32_t nj, int tid, int lane) {
  const uint32_t leaf_base = tw9_gadget_base(fgw, depth, 2);
  const uint32_t inner = w9_load(vals, lane);
  const uint32_t leaf_k1 = inner + w9_permute<FORM, false>(consts9, inner, 0u, nj, tid, lane, wl, leaf_base, 0u, dump);
  w9_store(wl, leaf_base + 364, leaf_k1, tid);
  uint32_t cur = tw9_second_half<FORM>(consts9, w9_load(vals + 9, lane), leaf_k1, nj, tid, lane, wl, leaf_base, leaf_base + 729, dump);
  // a level's second permutation, once per branch below as in k_tw9_chain: a k1 that was LOADED is waited for inside the round loop
  // (vmcnt(0) at its top, i.e. for the round's own stores too), and shared text would make the levels with a computed k1 pay that as well
  auto level_rest = [&](uint32_t r_in, uint32_t k1, uint32_t base, int l) -> uint32_t {
    if (l == depth - 1 && !root) return w9_permute<FORM, false>(consts9, r_in, k1, nj, tid, lane, wl, base + 365, 0u, dump);
    return tw9_second_half<FORM>(consts9, r_in, k1, nj, tid, lane, wl, base, l == depth - 1 ? 1u : base + 729, dump);
  };
#pragma unroll 1
  for (int l = 0; l < depth; l++) {
    const uint32_t base = tw9_gadget_base(fgw, depth, 4 + l);
    if ((index >> l) & 1) {  // the path node is the right input
      cur = level_rest(cur, w9_load(lvls + (size_t)l * 9, lane), base, l);
    } else {
      w9_store(wl, base - 1, cur, tid);  // `left` selector wire: the path node
      const uint32_t k1 = cur + w9_permute<FORM, false>(consts9, cur, 0u, nj, tid, lane, wl, base, 0u, dump);
      w9_store(wl, base + 364, k1, tid);
      cur = level_rest(w9_spread(fe_to_mont(fe_load<FrParams>(sibs + (size_t)l * 32)), lane), k1, base, l);
    }
  }
}

// the first permutation of a gadget whose left input is known before the walk (k_tw9_first, k_sw9_first, k_jw9_first): k1 = l + E_0(l)
// (< 4 N; form 2: < 10.5 N; lazy limbs) with its round wires at wbase (and at dup, if non-zero: a nullifier's, which is the left input of two gadgets),
// k1 into xch slot `slot`; selector: l is a level's sibling, which is also that level's `left` wire
template <int FORM>
__device__ __forceinline__ void w9_first_half(const uint32_t* __restrict__ consts9, const Fr& l_fe, uint32_t nj, int tid, int lane,
                                              uint32_t* __restrict__ wl, uint32_t wbase, uint32_t dup, bool selector, uint32_t* __restrict__ slot,
                                              uint32_t* __restrict__ dump) {
  const uint32_t l_in = w9_spread(l_fe, lane);
  if (selector) w9_store(wl, wbase - 1, l_in, tid);  // a level's `left` selector wire: the sibling
  const uint32_t k1 = l_in + (dup ? w9_permute<FORM, true>(consts9, l_in, 0u, nj, tid, lane, wl, wbase, dup, dump)
                                  : w9_permute<FORM, false>(consts9, l_in, 0u, nj, tid, lane, wl, wbase, 0u, dump));
  w9_store(wl, wbase + 364, k1, tid);
  if (dup) w9_store(wl, dup + 364, k1, tid);
  if (tid < 9) slot[lane] = k1;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_tw9_first(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int jobs = 7 + depth, tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / jobs;
  const int job = (int)(blockIdx.x % jobs);
  const uint8_t* in = inputs + g * (size_t)(T_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + TW9_XCH) * 9;
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + T_INDEX);
  if (job == 6 + depth) {  // the wires that are inputs, the square, the index bits and the 256 bit wires: lane-local values, a lane per wire
    const int lane = tid;
    const TransferChange chg = transfer_change(in);
    const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + T_CHAIN));
    if (lane == 0) w9_put_fe(wl, 0, Fr::one());
    if (lane == 1) w9_put_fe(wl, 3, chain_id);
    if (lane == 2) w9_put_fe(wl, 6, fe_to_mont(fe_load<FrParams>(in + T_NULLIFIER)));
    if (lane == 3) w9_put_fe(wl, 7, fe_to_mont(fe_load<FrParams>(in + T_SECRET)));
    if (lane == 4) w9_put_fe(wl, 8, fe_to_mont(fe_load<FrParams>(in + T_AMOUNT)));
    if (lane == 5) w9_put_fe(wl, 9, fe_to_mont(fe_load<FrParams>(in + T_TOKEN)));
    if (lane == 6) w9_put_fe(wl, 10, fe_to_mont(fe_load<FrParams>(in + T_PAY_COMMITMENT)));
    if (lane == 7) w9_put_fe(wl, 11, fe_to_mont(fe_load<FrParams>(in + T_PAY_AMOUNT)));
    if (lane == 8) w9_put_fe(wl, 12, fe_to_mont(fe_load<FrParams>(in + T_CHANGE_COMMITMENT)));
    if (lane == 9) w9_put_fe(wl, 13, chg.value());
    if (lane == 10) w9_put_fe(wl, 14 + 2 * depth, fe_sqr(chain_id));
    for (int l = lane; l < depth; l += 64) {
      w9_put_fe(wl, 14 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(T_REC + l) * 32)));
      w9_put_fe(wl, 14 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
    }
    for (int i = lane; i < 2 * T_BITS; i += 64) w9_put_fe(wl, 15 + 2 * depth + i, transfer_bit_wire(chg, i));
    return;
  }
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  // job 0 nullifier (gadget 0, the same wires again in gadget 3), 1 amount, 2 pay_amount, 3 change, 4 pay_commitment, 5 change_commitment
  Fr l_fe;
  uint32_t wbase, dup = 0;
  int slot;
  if (job >= 6) {
    const int lvl = job - 6;
    if (!((index >> lvl) & 1)) return;  // the path node is the LEFT input of this level: its first permutation is the chain's
    l_fe = fe_to_mont(fe_load<FrParams>(in + (size_t)(T_REC + lvl) * 32));
    wbase = tw9_gadget_base(fgw, depth, 4 + lvl);
    slot = lvl;
  } else {
    const int gadget = job < 2 ? job : job == 2 ? 4 + depth : job == 3 ? 6 + depth : job == 4 ? 5 + depth : 7 + depth;
    const int off = job == 0 ? T_NULLIFIER : job == 1 ? T_AMOUNT : job == 2 ? T_PAY_AMOUNT : job == 4 ? T_PAY_COMMITMENT : T_CHANGE_COMMITMENT;
    l_fe = job == 3 ? transfer_change(in).value() : fe_to_mont(fe_load<FrParams>(in + off));
    wbase = tw9_gadget_base(fgw, depth, gadget);
    if (job == 0) dup = tw9_gadget_base(fgw, depth, 3);
    slot = depth + (job < 2 ? job : job + 2);
  }
  w9_first_half<FORM>(consts9, l_fe, nj, tid, lane, wl, wbase, dup, job >= 6, xch + (size_t)slot * 9, xch + (size_t)(depth + TW9_DUMP) * 9);
}

template <int FORM>
__global__ void __launch_bounds__(64) k_tw9_second(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                  uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 5;
  const int job = (int)(blockIdx.x % 5);  // 0 inner, 1 asset, 2 nullifier_hash, 3 pay_asset, 4 change_asset
  const uint8_t* in = inputs + g * (size_t)(T_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + TW9_XCH) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const uint32_t k1 = w9_load(xch + (size_t)(depth + (job == 0 || job == 2 ? 0 : job == 1 ? 1 : job + 1)) * 9, lane);
  uint32_t r_in = 0;  // nullifier_hash = H(nullifier, 0)
  if (job == 0) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + T_SECRET)), lane);
  if (job == 1 || job >= 3) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + T_TOKEN)), lane);
  const uint32_t base = tw9_gadget_base(fgw, depth, job == 0 ? 0 : job == 1 ? 1 : job == 2 ? 3 : job == 3 ? 4 + depth : 6 + depth);
  const uint32_t hout = tw9_second_half<FORM>(consts9, r_in, k1, nj, tid, lane, wl, base, job == 2 ? 2u : base + 729, xch + (size_t)(depth + TW9_DUMP) * 9);
  if (job == 2) return;  // nullifier_hash: a public wire, nobody's input
  if (tid < 9) xch[(size_t)(depth + (job < 2 ? 2 + job : 5 + job)) * 9 + lane] = hout;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_tw9_chain(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 3;
  const int job = (int)(blockIdx.x % 3);  // 0 the chain, 1 pay_leaf, 2 change_leaf
  const uint8_t* in = inputs + g * (size_t)(T_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + TW9_XCH) * 9;
  uint32_t* dump = xch + (size_t)(depth + TW9_DUMP) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  if (job) {  // H(commitment, asset): E_0(commitment) and k1 are k_tw9_first's, the asset is k_tw9_second's
    const uint32_t base = tw9_gadget_base(fgw, depth, job == 1 ? 5 + depth : 7 + depth);
    tw9_second_half<FORM>(consts9, w9_load(xch + (size_t)(depth + 7 + job) * 9, lane), w9_load(xch + (size_t)(depth + 5 + job) * 9, lane), nj, tid,
                          lane, wl, base, 3u + (uint32_t)job, dump);
    return;
  }
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + T_INDEX);
  // H(l, r) with both permutations here (a level whose path node is the left input, and the leaf)
  auto hash_both = [&](uint32_t l_in, uint32_t r_in, uint32_t base, uint32_t out_wire) -> uint32_t {
    const uint32_t k1 = l_in + w9_permute<FORM, false>(consts9, l_in, 0u, nj, tid, lane, wl, base, 0u, dump);
    w9_store(wl, base + 364, k1, tid);
    return tw9_second_half<FORM>(consts9, r_in, k1, nj, tid, lane, wl, base, out_wire, dump);
  };
  const uint32_t leaf_base = tw9_gadget_base(fgw, depth, 2);
  uint32_t cur = hash_both(w9_load(xch + (size_t)(depth + 2) * 9, lane), w9_load(xch + (size_t)(depth + 3) * 9, lane), leaf_base, leaf_base + 729);
#pragma unroll 1
  for (int l = 0; l < depth; l++) {
    const uint32_t base = tw9_gadget_base(fgw, depth, 4 + l);
    const uint32_t out_wire = l == depth - 1 ? 1u : base + 729;
    if ((index >> l) & 1) {  // the path node is the right input: E_0(sibling), k1 and the selector wire are k_tw9_first's
      cur = tw9_second_half<FORM>(consts9, cur, w9_load(xch + (size_t)l * 9, lane), nj, tid, lane, wl, base, out_wire, dump);
    } else {
      w9_store(wl, base - 1, cur, tid);  // `left` selector wire: the path node
      cur = hash_both(cur, w9_spread(fe_to_mont(fe_load<FrParams>(in + (size_t)(T_REC + l) * 32)), lane), base, out_wire);
    }
  }
}

// Boundary check of the transfer records, one lane per field as k_check_split_records: every field canonical (< r), the index inside
// the tree, amount < 2^128 (field 2), pay_amount < 2^128 and pay_amount <= amount (field 7) -- compared on the integer words, not in
// the field.  bad[g] = lowest offending field of record g (the caller initialises it to 0xffffffff): 0 nullifier, 1 secret, 2 amount,
// 3 index, 4 token, 5 chain_id, 6 pay_commitment, 7 pay_amount, 8 change_commitment, 9 + l sibling l.
__global__ void __launch_bounds__(64) k_check_transfer_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(T_REC + depth)) return;
  const uint8_t* rec = inputs + g * (size_t)(T_REC + depth) * 32;
  const uint8_t* p = rec + (size_t)f * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 2 || f == 7) ok = ok && rec_amount_ok(w);
  if (f == 7) ok = ok && rec_le(w, reinterpret_cast<const uint32_t*>(rec + T_AMOUNT));  // pay_amount <= amount
  if (f == 3) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void transfer_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_transfer_records, dim3(grid_for(T_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream, inputs_d, a.depth, n, bad_d);
}

static void transfer_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_transfer_core, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, inputs_d, depth,
                     (size_t)s.n_wires, (uint32_t)s.first_bit_wire, n, out_d);
}

static void transfer_launch_w9(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint32_t* wl, uint32_t* xch) {
  const uint32_t* c9 = (const uint32_t*)ctx->mimc_consts9_d;
  OG_W9_LAUNCH(k_tw9_first, w9_rows(), dim3((unsigned)(n * (size_t)(7 + depth))), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires,
               (uint32_t)s.first_gadget_wire, wl, xch);
  OG_W9_LAUNCH(k_tw9_second, w9_rows(), dim3((unsigned)(n * 5)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires,
               (uint32_t)s.first_gadget_wire, wl, xch);
  OG_W9_LAUNCH(k_tw9_chain, w9_rows(), dim3((unsigned)(n * 3)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires,
               (uint32_t)s.first_gadget_wire, wl, xch);
}

// ---- the wave-wide walk of the split and the join statement ---------------------------------------------------------------------------
// The same decomposition as k_tw9_* (its header: ONE permutation per one-wave workgroup, three launches, values between them as nine
// lazy limbs in xch, wires as nine limbs in wl for k_wires_from_limbs, every hash output through w9_renorm before it is anybody's
// input, unconditional stores with a dump slot for the lanes without a limb).  split's gadgets lie exactly where transfer's first
// 6 + depth lie (change_asset, change_leaf where pay_asset, pay_leaf are), so tw9_gadget_base serves it as it is; a join note's
// gadgets are a transfer's first 4 + depth from the note's own first wire, and the two output gadgets follow note b's levels as
// gadgets 4 + depth and 5 + depth of note b would.  The bodies the three statements share are above k_tw9_first: tw9_second_half,
// w9_first_half, w9_note_chain.
//
// split:
//   k_sw9_first   grid n x (5 + depth): E_0 of nullifier (wires of gadgets 0 and 3), amount, change (from the record's integer words,
//                 as k_split_core) and change_commitment; E_0(sibling_l) of every level whose path node is the RIGHT input; one
//                 workgroup for the wires that are inputs, the two squares, the index bits and the 256 bit wires
//   k_sw9_second  grid n x 4: the second permutations of inner, asset, nullifier_hash (-> wire 2), change_asset
//   k_sw9_chain   grid n x 2: block 0 is the chain (leaf, then the levels: k_w9_chain's work, exactly as long as withdraw's); block 1
//                 is the second permutation of change_leaf (-> wire 7)
// xch slots per request beyond the levels: [depth + 0] k1 of inner / nullifier_hash, [1] k1 of asset, [2] inner, [3] asset, [4] k1 of
// change_asset, [5] k1 of change_leaf, [6] change_asset, [7 .. 10]: 36 words nobody reads -- where the lanes without a limb store
// (w9_permute `dump`)
constexpr int SW9_XCH = 11, SW9_DUMP = 7;
// amount_out and change = amount - amount_out as 64-bit halves (transfer's pair: p is what leaves the note, c what stays)
__device__ __forceinline__ TransferChange split_change(const uint8_t* in) {
  const uint64_t a_lo = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT), a_hi = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT + 8);
  TransferChange c;
  c.p_lo = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT_OUT);
  c.p_hi = *reinterpret_cast<const uint64_t*>(in + S_AMOUNT_OUT + 8);
  c.c_lo = a_lo - c.p_lo;
  c.c_hi = a_hi - c.p_hi - (a_lo < c.p_lo ? 1u : 0u);
  return c;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_sw9_first(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int jobs = 5 + depth, tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / jobs;
  const int job = (int)(blockIdx.x % jobs);
  const uint8_t* in = inputs + g * (size_t)(S_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + SW9_XCH) * 9;
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + S_INDEX);
  if (job == 4 + depth) {  // the wires that are inputs, the squares, the index bits and the 256 bit wires: lane-local values, a lane per wire
    const int lane = tid;
    const TransferChange chg = split_change(in);
    const Fr recipient = fe_to_mont(fe_load<FrParams>(in + S_RECIPIENT)), chain_id = fe_to_mont(fe_load<FrParams>(in + S_CHAIN));
    if (lane == 0) w9_put_fe(wl, 0, Fr::one());
    if (lane == 1) w9_put_fe(wl, 3, recipient);
    if (lane == 2) w9_put_fe(wl, 4, fe_to_mont(fe_load<FrParams>(in + S_AMOUNT_OUT)));
    if (lane == 3) w9_put_fe(wl, 5, fe_to_mont(fe_load<FrParams>(in + S_TOKEN)));
    if (lane == 4) w9_put_fe(wl, 6, chain_id);
    if (lane == 5) w9_put_fe(wl, 8, fe_to_mont(fe_load<FrParams>(in + S_NULLIFIER)));
    if (lane == 6) w9_put_fe(wl, 9, fe_to_mont(fe_load<FrParams>(in + S_SECRET)));
    if (lane == 7) w9_put_fe(wl, 10, fe_to_mont(fe_load<FrParams>(in + S_AMOUNT)));
    if (lane == 8) w9_put_fe(wl, 11, fe_to_mont(fe_load<FrParams>(in + S_CHANGE_COMMITMENT)));
    if (lane == 9) w9_put_fe(wl, 12, chg.value());
    if (lane == 10) w9_put_fe(wl, 13 + 2 * depth, fe_sqr(recipient));
    if (lane == 11) w9_put_fe(wl, 14 + 2 * depth, fe_sqr(chain_id));
    for (int l = lane; l < depth; l += 64) {
      w9_put_fe(wl, 13 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(S_REC + l) * 32)));
      w9_put_fe(wl, 13 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
    }
    for (int i = lane; i < 2 * S_BITS; i += 64) w9_put_fe(wl, 15 + 2 * depth + i, transfer_bit_wire(chg, i));  // amount_out, then change
    return;
  }
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  // job 0 nullifier (gadget 0, the same wires again in gadget 3), 1 amount, 2 change, 3 change_commitment, 4 + l sibling l
  Fr l_fe;
  uint32_t wbase, dup = 0;
  int slot;
  if (job >= 4) {
    const int lvl = job - 4;
    if (!((index >> lvl) & 1)) return;  // the path node is the LEFT input of this level: its first permutation is the chain's
    l_fe = fe_to_mont(fe_load<FrParams>(in + (size_t)(S_REC + lvl) * 32));
    wbase = tw9_gadget_base(fgw, depth, 4 + lvl);
    slot = lvl;
  } else {
    l_fe = job == 2 ? split_change(in).value() : fe_to_mont(fe_load<FrParams>(in + (job == 0 ? S_NULLIFIER : job == 1 ? S_AMOUNT : S_CHANGE_COMMITMENT)));
    wbase = tw9_gadget_base(fgw, depth, job < 2 ? job : 2 + depth + job);
    if (job == 0) dup = tw9_gadget_base(fgw, depth, 3);
    slot = depth + (job < 2 ? job : job + 2);
  }
  w9_first_half<FORM>(consts9, l_fe, nj, tid, lane, wl, wbase, dup, job >= 4, xch + (size_t)slot * 9, xch + (size_t)(depth + SW9_DUMP) * 9);
}

template <int FORM>
__global__ void __launch_bounds__(64) k_sw9_second(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                  uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 4;
  const int job = (int)(blockIdx.x % 4);  // 0 inner, 1 asset, 2 nullifier_hash, 3 change_asset
  const uint8_t* in = inputs + g * (size_t)(S_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + SW9_XCH) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const uint32_t k1 = w9_load(xch + (size_t)(depth + (job == 1 ? 1 : job == 3 ? 4 : 0)) * 9, lane);
  uint32_t r_in = 0;  // nullifier_hash = H(nullifier, 0)
  if (job == 0) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + S_SECRET)), lane);
  if (job == 1 || job == 3) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + S_TOKEN)), lane);
  const uint32_t base = tw9_gadget_base(fgw, depth, job == 2 ? 3 : job == 3 ? 4 + depth : job);
  const uint32_t hout = tw9_second_half<FORM>(consts9, r_in, k1, nj, tid, lane, wl, base, job == 2 ? 2u : base + 729, xch + (size_t)(depth + SW9_DUMP) * 9);
  if (job == 2) return;  // nullifier_hash: a public wire, nobody's input
  if (tid < 9) xch[(size_t)(depth + (job < 2 ? 2 + job : 6)) * 9 + lane] = hout;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_sw9_chain(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 2;
  const uint8_t* in = inputs + g * (size_t)(S_REC + depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(depth + SW9_XCH) * 9;
  uint32_t* dump = xch + (size_t)(depth + SW9_DUMP) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  if (blockIdx.x & 1) {  // change_leaf = H(change_commitment, change_asset): k1 is k_sw9_first's, the asset is k_sw9_second's
    tw9_second_half<FORM>(consts9, w9_load(xch + (size_t)(depth + 6) * 9, lane), w9_load(xch + (size_t)(depth + 5) * 9, lane), nj, tid, lane, wl,
                          tw9_gadget_base(fgw, depth, 5 + depth), 7u, dump);
    return;
  }
  w9_note_chain<FORM>(consts9, in + (size_t)S_REC * 32, *reinterpret_cast<const uint64_t*>(in + S_INDEX), depth, fgw, true, wl, xch,
                      xch + (size_t)(depth + 2) * 9, dump, nj, tid, lane);
}

// The wave-wide walk of n split requests.  wl is n x n_wires x 36 B from the arena: 0.52 GB for 512 depth-32 requests (28 104 wires
// each), the largest call that takes this walk by default.
static void split_launch_w9(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint32_t* wl, uint32_t* xch) {
  const uint32_t* c9 = (const uint32_t*)ctx->mimc_consts9_d;
  const uint32_t fgw = (uint32_t)s.first_gadget_wire;
  OG_W9_LAUNCH(k_sw9_first, w9_rows(), dim3((unsigned)(n * (size_t)(5 + depth))), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires, fgw,
               wl, xch);
  OG_W9_LAUNCH(k_sw9_second, w9_rows(), dim3((unsigned)(n * 4)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires, fgw, wl, xch);
  OG_W9_LAUNCH(k_sw9_chain, w9_rows(), dim3((unsigned)(n * 2)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires, fgw, wl, xch);
}

// join:
//   k_jw9_first   grid n x (7 + 2 depth): E_0 of nullifier_a and nullifier_b (each into its note's gadgets 0 and 3), amount_a, amount_b,
//                 sum (from the record's integer words, as k_join_core) and out_commitment; E_0(sibling) of every level of either
//                 walk whose path node is the RIGHT input; one workgroup for the wires that are inputs, chain_id^2, the index bits
//                 and the 384 bit wires
//   k_jw9_second  grid n x 7: the second permutations of inner, asset and nullifier_hash of note a (-> wire 2) and of note b (-> wire
//                 3), and of out_asset.  Both nullifier hashes go into xch as well: they are the inputs of nh_diff_inv
//   k_jw9_chain   grid n x 4: block 0 is note a's chain, block 1 note b's -- side by side, each as long as withdraw's; wire 1 comes from
//                 note a's walk ALONE (note b's last level stores its round wires and no output), so a record whose two paths do
//                 not meet carries note a's root and the prover's row check refuses it (tests/join_cases.py case_different_roots);
//                 block 2 is the second permutation of out_leaf (-> wire 5); block 3 is nh_diff_inv = 1 / (nullifier_hash_a -
//                 nullifier_hash_b) -> wire 15, ONE lane-local fe_inv on one lane: ~380 products beside a chain of ~19 000, not
//                 worth spreading (k_join_core says the same of its own)
// xch slots per request: [0 .. depth) k1 of note a's levels, [depth .. 2 depth) of note b's; beyond them [2 depth + 0] k1 of inner_a /
// nullifier_hash_a, [1] k1 of asset_a, [2] inner_a, [3] asset_a, [4] nullifier_hash_a, [5 .. 9] the same five of note b, [10] k1 of
// out_asset, [11] k1 of out_leaf, [12] out_asset, [13 .. 16]: 36 words nobody reads -- where the lanes without a limb store
// (w9_permute `dump`)
constexpr int JW9_XCH = 17, JW9_NOTE = 5, JW9_OUT = 10, JW9_DUMP = 13;
constexpr int J_NOTE_BYTES = 128, J_NULLIFIER = 0, J_SECRET = 32, J_AMOUNT = 64, J_INDEX = 96;  // a note's fields, from the note's first byte
constexpr int J_TOKEN = 256, J_CHAIN = 288, J_OUT_COMMITMENT = 320;
// amount_a, amount_b and sum = amount_a + amount_b on the record's integer words (the records are checked first: the sum is below
// 2^128), as 64-bit words: a_lo a_hi b_lo b_hi s_lo s_hi
struct JoinSum {
  uint64_t w[6];
  __device__ __forceinline__ Fr value() const {
    const uint32_t sw[8] = {(uint32_t)w[4], (uint32_t)(w[4] >> 32), (uint32_t)w[5], (uint32_t)(w[5] >> 32), 0u, 0u, 0u, 0u};
    return fe_to_mont(fe_from_words<FrParams>(sw));
  }
  // bit i (0 .. 383) of amount_a | amount_b | sum, as a wire
  __device__ __forceinline__ Fr bit_wire(int i) const {
    uint64_t word = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) word = (i >> 6) == k ? w[k] : word;
    return ((word >> (i & 63)) & 1) ? Fr::one() : Fr::zero();
  }
};
__device__ __forceinline__ JoinSum join_sum(const uint8_t* in) {
  JoinSum s;
  s.w[0] = *reinterpret_cast<const uint64_t*>(in + J_AMOUNT);
  s.w[1] = *reinterpret_cast<const uint64_t*>(in + J_AMOUNT + 8);
  s.w[2] = *reinterpret_cast<const uint64_t*>(in + J_NOTE_BYTES + J_AMOUNT);
  s.w[3] = *reinterpret_cast<const uint64_t*>(in + J_NOTE_BYTES + J_AMOUNT + 8);
  s.w[4] = s.w[0] + s.w[2];
  s.w[5] = s.w[1] + s.w[3] + (s.w[4] < s.w[0] ? 1u : 0u);
  return s;
}

template <int FORM>
__global__ void __launch_bounds__(64) k_jw9_first(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t ngw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int jobs = 7 + 2 * depth, tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / jobs;
  const int job = (int)(blockIdx.x % jobs);
  const uint8_t* in = inputs + g * (size_t)(J_REC + 2 * depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(2 * depth + JW9_XCH) * 9;
  if (job == 6 + 2 * depth) {  // the wires that are inputs, the square, the index bits and the 384 bit wires: lane-local values, a lane per wire
    const int lane = tid;
    const JoinSum sum = join_sum(in);
    const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + J_CHAIN));
    if (lane == 0) w9_put_fe(wl, 0, Fr::one());
    if (lane == 1) w9_put_fe(wl, 4, chain_id);
    if (lane >= 2 && lane < 8) {  // 6 nullifier_a | 7 secret_a | 8 amount_a | 9 nullifier_b | 10 secret_b | 11 amount_b
      const int f = lane - 2;
      w9_put_fe(wl, 4 + lane, fe_to_mont(fe_load<FrParams>(in + (size_t)(f / 3) * J_NOTE_BYTES + (size_t)(f % 3) * 32)));
    }
    if (lane == 8) w9_put_fe(wl, 12, fe_to_mont(fe_load<FrParams>(in + J_TOKEN)));
    if (lane == 9) w9_put_fe(wl, 13, fe_to_mont(fe_load<FrParams>(in + J_OUT_COMMITMENT)));
    if (lane == 10) w9_put_fe(wl, 14, sum.value());
    if (lane == 11) w9_put_fe(wl, 16 + 4 * depth, fe_sqr(chain_id));
    for (int l = lane; l < 2 * depth; l += 64) {  // siblings_a | siblings_b, then the index bits of a | b
      const int b = l >= depth ? 1 : 0, lvl = l - b * depth;
      const uint64_t index = *reinterpret_cast<const uint64_t*>(in + (size_t)b * J_NOTE_BYTES + J_INDEX);
      w9_put_fe(wl, 16 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(J_REC + l) * 32)));
      w9_put_fe(wl, 16 + 2 * depth + l, ((index >> lvl) & 1) ? Fr::one() : Fr::zero());
    }
    for (int i = lane; i < 3 * J_BITS; i += 64) w9_put_fe(wl, 17 + 4 * depth + i, sum.bit_wire(i));
    return;
  }
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  // job 0 nullifier_a (gadget 0 of note a, the same wires again in its gadget 3), 1 amount_a, 2 nullifier_b, 3 amount_b, 4 sum (out_asset),
  // 5 out_commitment (out_leaf), 6 + l sibling l of note a, 6 + depth + l sibling l of note b
  Fr l_fe;
  uint32_t wbase, dup = 0;
  int slot;
  if (job >= 6) {
    const int b = job - 6 >= depth ? 1 : 0, lvl = job - 6 - b * depth;
    const uint64_t index = *reinterpret_cast<const uint64_t*>(in + (size_t)b * J_NOTE_BYTES + J_INDEX);
    if (!((index >> lvl) & 1)) return;  // the path node is the LEFT input of this level: its first permutation is the chain's
    l_fe = fe_to_mont(fe_load<FrParams>(in + (size_t)(J_REC + b * depth + lvl) * 32));
    wbase = tw9_gadget_base(fgw + (uint32_t)b * ngw, depth, 4 + lvl);
    slot = b * depth + lvl;
  } else if (job >= 4) {
    l_fe = job == 4 ? join_sum(in).value() : fe_to_mont(fe_load<FrParams>(in + J_OUT_COMMITMENT));
    wbase = tw9_gadget_base(fgw + ngw, depth, depth + job);  // behind note b's levels: gadgets 4 + depth and 5 + depth from note b's first wire
    slot = 2 * depth + JW9_OUT + (job - 4);
  } else {
    const int b = job >> 1, f = job & 1;  // f = 0 the nullifier, 1 the amount
    l_fe = fe_to_mont(fe_load<FrParams>(in + (size_t)b * J_NOTE_BYTES + (f ? J_AMOUNT : J_NULLIFIER)));
    wbase = tw9_gadget_base(fgw + (uint32_t)b * ngw, depth, f);
    if (!f) dup = tw9_gadget_base(fgw + (uint32_t)b * ngw, depth, 3);
    slot = 2 * depth + b * JW9_NOTE + f;
  }
  w9_first_half<FORM>(consts9, l_fe, nj, tid, lane, wl, wbase, dup, job >= 6, xch + (size_t)slot * 9, xch + (size_t)(2 * depth + JW9_DUMP) * 9);
}

template <int FORM>
__global__ void __launch_bounds__(64) k_jw9_second(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                  uint32_t fgw, uint32_t ngw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 7;
  const int job = (int)(blockIdx.x % 7);  // 0 inner_a, 1 asset_a, 2 nullifier_hash_a, 3 .. 5 the same of note b, 6 out_asset
  const uint8_t* in = inputs + g * (size_t)(J_REC + 2 * depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(2 * depth + JW9_XCH) * 9;
  uint32_t* vals = xch + (size_t)(2 * depth) * 9;
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  const Fr token = fe_to_mont(fe_load<FrParams>(in + J_TOKEN));
  if (job == 6) {  // out_asset = H(sum, token)
    const uint32_t base = tw9_gadget_base(fgw + ngw, depth, 4 + depth);
    const uint32_t hout = tw9_second_half<FORM>(consts9, w9_spread(token, lane), w9_load(vals + (size_t)JW9_OUT * 9, lane), nj, tid, lane, wl, base,
                                                base + 729, vals + (size_t)JW9_DUMP * 9);
    if (tid < 9) vals[(size_t)(JW9_OUT + 2) * 9 + lane] = hout;
    return;
  }
  const int b = job >= 3 ? 1 : 0, h = job - 3 * b;  // 0 inner, 1 asset, 2 nullifier_hash of note b
  uint32_t* note = vals + (size_t)(b * JW9_NOTE) * 9;
  const uint32_t k1 = w9_load(note + (size_t)(h == 1 ? 1 : 0) * 9, lane);
  uint32_t r_in = 0;  // nullifier_hash = H(nullifier, 0)
  if (h == 0) r_in = w9_spread(fe_to_mont(fe_load<FrParams>(in + (size_t)b * J_NOTE_BYTES + J_SECRET)), lane);
  if (h == 1) r_in = w9_spread(token, lane);
  const uint32_t base = tw9_gadget_base(fgw + (uint32_t)b * ngw, depth, h == 2 ? 3 : h);
  const uint32_t hout = tw9_second_half<FORM>(consts9, r_in, k1, nj, tid, lane, wl, base, h == 2 ? 2u + (uint32_t)b : base + 729,
                                              vals + (size_t)JW9_DUMP * 9);
  if (tid < 9) note[(size_t)(2 + h) * 9 + lane] = hout;  // (the nullifier hash too: nh_diff_inv reads it)
}

template <int FORM>
__global__ void __launch_bounds__(64) k_jw9_chain(const uint32_t* __restrict__ consts9, const uint8_t* __restrict__ inputs, int depth, size_t n_wires,
                                                 uint32_t fgw, uint32_t ngw, uint32_t* __restrict__ wl_all, uint32_t* __restrict__ xch_all) {
  OG_FILLER_PRIO();
  const int tid = threadIdx.x, lane = FORM ? w9_row_limb(tid) : tid;
  const size_t g = blockIdx.x / 4;
  const int job = (int)(blockIdx.x % 4);  // 0 note a's chain, 1 note b's, 2 out_leaf, 3 nh_diff_inv
  const uint8_t* in = inputs + g * (size_t)(J_REC + 2 * depth) * 32;
  uint32_t* wl = wl_all + g * n_wires * 9;
  uint32_t* xch = xch_all + g * (size_t)(2 * depth + JW9_XCH) * 9;
  uint32_t* vals = xch + (size_t)(2 * depth) * 9;
  uint32_t* dump = vals + (size_t)JW9_DUMP * 9;
  if (job == 3) {  // lane-local, one lane: both hashes are below 2 N with limbs < 2^29 + 32 (w9_renorm); fe_sub wants normalized limbs
    if (tid) return;
    uint32_t ta[9], tb[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      ta[i] = vals[(size_t)4 * 9 + i];
      tb[i] = vals[(size_t)(JW9_NOTE + 4) * 9 + i];
    }
    w9_put_fe(wl, 15, fe_inv(fe_sub(fe_from_lazy_limbs<FrParams>(ta), fe_from_lazy_limbs<FrParams>(tb))));  // a - b, never b - a
    return;
  }
  const uint32_t nj = w9_modulus_limb<FrParams>(lane);
  if (job == 2) {  // out_leaf = H(out_commitment, out_asset): k1 is k_jw9_first's, the asset is k_jw9_second's
    tw9_second_half<FORM>(consts9, w9_load(vals + (size_t)(JW9_OUT + 2) * 9, lane), w9_load(vals + (size_t)(JW9_OUT + 1) * 9, lane), nj, tid, lane, wl,
                          tw9_gadget_base(fgw + ngw, depth, 5 + depth), 5u, dump);
    return;
  }
  const uint8_t* note = in + (size_t)job * J_NOTE_BYTES;
  w9_note_chain<FORM>(consts9, in + (size_t)(J_REC + job * depth) * 32, *reinterpret_cast<const uint64_t*>(note + J_INDEX), depth,
                      fgw + (uint32_t)job * ngw, job == 0, wl, xch + (size_t)(job * depth) * 9, vals + (size_t)(job * JW9_NOTE + 2) * 9, dump, nj, tid,
                      lane);
}

// The wave-wide walk of n join requests.  wl is n x n_wires x 36 B from the arena: 1.0 GB for 512 depth-32 requests (54 608 wires each),
// the largest call that takes this walk by default.
static void join_launch_w9(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint32_t* wl, uint32_t* xch) {
  const uint32_t* c9 = (const uint32_t*)ctx->mimc_consts9_d;
  const uint32_t fgw = (uint32_t)s.first_gadget_wire, ngw = (uint32_t)s.note_gadget_wires;
  OG_W9_LAUNCH(k_jw9_first, w9_rows(), dim3((unsigned)(n * (size_t)(7 + 2 * depth))), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires,
               fgw, ngw, wl, xch);
  OG_W9_LAUNCH(k_jw9_second, w9_rows(), dim3((unsigned)(n * 7)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires, fgw, ngw, wl, xch);
  OG_W9_LAUNCH(k_jw9_chain, w9_rows(), dim3((unsigned)(n * 4)), dim3(64), 0, ctx->stream, c9, inputs_d, depth, (size_t)s.n_wires, fgw, ngw, wl, xch);
}

// ---- the claim statement: an owned note into an ordinary note of the same value ---------------------------------------------------------
// Spec: tests/claim_spec.py.  public: root, nullifier_hash, chain_id, out_leaf (n_pub = 4); private: x, amount, token, out_commitment,
// the path.  An owned note (notes.hip, og_note_seal_owned_batch_d) is bound to a one-time key P = pk + t BASE of which only the payee
// knows the discrete logarithm x = sk + t mod l; the sender, who knows everything else about the note, cannot spend it.  x = sum 2^i b_i
// over 251 boolean wires with x < l (l the order of BASE: without the bound x + l is a second key with another nullifier hash);
// P = x BASE; c = H(P.x, P.y); asset = H(amount, token); leaf = H(c, asset) lies under root; nullifier_hash = H(x, 1) (an ordinary
// spend publishes H(nullifier, 0)); out_leaf = H(out_commitment, asset) -- the SAME asset wire, a leaf of the deposit shape.  No
// reference counterpart (the snapshot has no circuit).
// Input record per request, (6 + depth) x 32 B canonical LE:
//   x | amount | token | chain_id | out_commitment | index (u64 in the low bytes) | siblings[depth]
// Wires:
//   0 one | 1 root | 2 nullifier_hash | 3 chain_id | 4 out_leaf | 5 x | 6 amount | 7 token | 8 out_commitment
//   9.. siblings[D] | index bits[D] | chain_id^2 | x bits[251] (LSB first) | the comparison's 114 wires t (one per 1-bit of l - 1, most
//   significant first: t = "x equals l - 1 on every bit so far") | the multiplication's wires, per bit w1 = b x1, w2 = b y1, w3 = w1 y1,
//   x3, y3 with (x1, y1) the partial sum before the bit and (x3, y3) after it | the gadgets: c, asset, leaf, nullifier_hash (out =
//   wire 2), level 0..D-1 (the last one's out = wire 1), out_leaf (out = wire 4)
// One walk: k_claim_core, one lane per request.  NOT built for this statement: a wave-wide walk, host chains.
constexpr int C_PUB = 4;
constexpr int C_REC = 6;  // fields of a claim record before the siblings
constexpr int C_BITS = EdOrder::BITS, C_CMP = 114;
// byte offsets of the record's fields
constexpr int C_X = 0, C_AMOUNT = 32, C_TOKEN = 64, C_CHAIN = 96, C_OUT_COMMITMENT = 128, C_INDEX = 160;

static RecordShape claim_shape(const StatementArgs& a) {
  RecordShape s{};
  const int depth = a.depth;
  const uint64_t hashes = 5 + (uint64_t)depth;
  s.first_bit_wire = 1 + C_PUB + 4 + 2 * (uint64_t)depth + 1;
  s.first_gadget_wire = s.first_bit_wire + C_BITS + C_CMP + 5 * C_BITS;
  s.n_wires = s.first_gadget_wire + depth + hashes * 730 - 3;  // a `left` per level; nullifier_hash, root and out_leaf are public wires
  s.n_constraints = 3 + C_BITS + 6 * C_BITS + 2 * (uint64_t)depth + hashes * 730;
  return s;
}

// bit i of the record's x (the records are checked first: x < l < 2^251), read from the record: no register array is indexed
__device__ __forceinline__ bool claim_x_bit(const uint8_t* in, int i) {
  return ((reinterpret_cast<const uint32_t*>(in + C_X)[i >> 5] >> (i & 31)) & 1u) != 0;
}

// One lane per request, as k_transfer_core: the (5 + depth) MultiMiMC7 gadgets through the one rolled permutation body (gadget_wires);
// Montgomery values are stored and k_wires_from_mont converts them afterwards, in parallel.  The wires of the key -- the bits of x, the
// comparison, the multiplication -- are owned_key_wires, which k_send_core and k_redeem_core call too (further down).
// The multiplication's wires are the 251 AFFINE partial sums S_1 .. S_251 of x BASE, bit 0 first.  Two inversions per bit would be ~10^5
// products a request against ~2.7 10^4 for the 37 hashes; instead the sum is walked projectively through the one addition site of the
// unified law (the addend taken from the 64 x 16 table of BASE under a select on the bit, as the seal's ladder takes its own: entry
// d = 2^(i mod 4) of window i / 4 is 2^i BASE) and every step PARKS what the way back needs in its own wire slots of the output row:
//     slot w1 <- Z_1 Z_2 .. Z_(i+1), the running product;  w2 <- Z_(i+1);  x3 <- X_(i+1);  y3 <- Y_(i+1)      (w3 stays free)
// One inversion of the last running product (Montgomery's trick), then the slots are passed backwards: step i reads the running
// product of step i - 1, forms 1 / Z_(i+1) and the affine S_(i+1), stores x3 and y3 of its own step and w1, w2, w3 of step i + 1,
// whose parked values the previous iteration has consumed.  No scratch buffer beyond the witness, no runtime-indexed register array.
// Z never vanishes: the law is complete on the curve.
// in: the record, whose field 0 is x in all three owned statements; z: the request's witness row; ww: the writer, whose cursor stands
// at the first bit wire of x and is left behind the multiplication's last wire; (px, py) <- P = x BASE, affine
__device__ __forceinline__ void owned_key_wires(const uint8_t* __restrict__ tab, const uint8_t* in, uint8_t* z, WireWriterT<false>& ww, Fr& px, Fr& py) {
#pragma unroll 1
  for (int i = 0; i < C_BITS; i++) ww.push(claim_x_bit(in, i) ? Fr::one() : Fr::zero());
  {  // the comparison with l - 1, most significant bit first: a wire per 1-bit of l - 1 (wave-uniform: a constant)
    bool t = true;
#pragma unroll 1
    for (int i = C_BITS - 1; i >= 0; i--) {
      if (ed_order_minus_1_bit(i)) {
        t = t && claim_x_bit(in, i);
        ww.push(t ? Fr::one() : Fr::zero());
      }
    }
  }
  {
    const Fr ca = ed_const(168700), cd = ed_const(168696);
    uint8_t* mul = z + (size_t)ww.w * 32;  // step i: w1 | w2 | w3 | x3 | y3 at mul + 160 i
    EdPoint acc = ed_identity();
    Fr run = Fr::one();
#pragma unroll 1
    for (int i = 0; i < C_BITS; i++) {
      const bool b = claim_x_bit(in, i);
      const uint8_t* e = tab + (size_t)((i >> 2) * ED_TAB_DIGITS + (1 << (i & 3))) * 64;
      const Fr tx = fe_load<FrParams>(e), ty = fe_load<FrParams>(e + 32);
      EdPoint q = ed_identity();
#pragma unroll
      for (int k = 0; k < 9; k++) {
        q.x.l[k] = b ? tx.l[k] : q.x.l[k];
        q.y.l[k] = b ? ty.l[k] : q.y.l[k];
      }
      acc = ed_add(acc, q, ca, cd);
      run = fe_mul(run, acc.z);
      uint8_t* slot = mul + (size_t)i * 160;
      fe_store(slot, run);
      fe_store(slot + 32, acc.z);
      fe_store(slot + 96, acc.x);
      fe_store(slot + 128, acc.y);
    }
    Fr inv = fe_inv(run);
    px = Fr::zero();
    py = Fr::one();
#pragma unroll 1
    for (int i = C_BITS - 1; i >= 0; i--) {
      uint8_t* slot = mul + (size_t)i * 160;
      const Fr before = i ? fe_load<FrParams>(slot - 160) : Fr::one();  // Z_1 .. Z_i
      const Fr zi = fe_mul(inv, before);                                // 1 / Z_(i+1)
      inv = fe_mul(inv, fe_load<FrParams>(slot + 32));
      const Fr sx = fe_mul(fe_load<FrParams>(slot + 96), zi), sy = fe_mul(fe_load<FrParams>(slot + 128), zi);
      fe_store(slot + 96, sx);
      fe_store(slot + 128, sy);
      if (i == C_BITS - 1) {
        px = sx;
        py = sy;
      } else {  // S_(i+1) is what step i + 1 starts from
        const bool b = claim_x_bit(in, i + 1);
        const Fr sxy = fe_mul(sx, sy);
        fe_store(slot + 160, b ? sx : Fr::zero());
        fe_store(slot + 192, b ? sy : Fr::zero());
        fe_store(slot + 224, b ? sxy : Fr::zero());
      }
    }
    // step 0 starts from (0, 1)
    fe_store(mul, Fr::zero());
    fe_store(mul + 32, claim_x_bit(in, 0) ? Fr::one() : Fr::zero());
    fe_store(mul + 64, Fr::zero());
    ww.w += 5 * C_BITS;
  }
}

__global__ void __launch_bounds__(64) k_claim_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const uint8_t* __restrict__ inputs,
                                                  int depth, size_t n_wires, uint32_t first_bit_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(C_REC + depth) * 32;
  uint8_t* z = out + g * n_wires * 32;
  WireWriterT<false> ww{z, first_bit_wire};
  const Fr x = fe_to_mont(fe_load<FrParams>(in + C_X));
  const Fr amount = fe_to_mont(fe_load<FrParams>(in + C_AMOUNT));
  const Fr token = fe_to_mont(fe_load<FrParams>(in + C_TOKEN));
  const Fr chain_id = fe_to_mont(fe_load<FrParams>(in + C_CHAIN));
  const Fr out_commitment = fe_to_mont(fe_load<FrParams>(in + C_OUT_COMMITMENT));
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + C_INDEX);
  ww.put(0, Fr::one());
  ww.put(3, chain_id);
  ww.put(5, x);
  ww.put(6, amount);
  ww.put(7, token);
  ww.put(8, out_commitment);
  for (int l = 0; l < depth; l++) {
    ww.put(9 + l, fe_to_mont(fe_load<FrParams>(in + (size_t)(C_REC + l) * 32)));
    ww.put(9 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
  }
  ww.put(9 + 2 * depth, fe_sqr(chain_id));
  Fr px, py;  // P = x BASE, affine
  owned_key_wires(tab, in, z, ww, px, py);
  // gadget 0: c = H(P.x, P.y); 1: asset = H(amount, token); 2: leaf = H(c, asset); 3: nullifier_hash = H(x, 1) -> wire 2; 4 + l: level
  // l of the path (wire 1 = root for the last level); 4 + depth: out_leaf = H(out_commitment, asset) -> wire 4
  Fr cur = Fr::zero(), c = Fr::zero(), asset = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 5 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = px; r_in = py;
    } else if (h == 1) {
      l_in = amount; r_in = token;
    } else if (h == 2) {
      l_in = c; r_in = asset;
    } else if (h == 3) {
      l_in = x; r_in = Fr::one(); out_wire = 2;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = fe_to_mont(fe_load<FrParams>(in + (size_t)(C_REC + lvl) * 32));
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    } else {
      l_in = out_commitment; r_in = asset; out_wire = 4;
    }
    const Fr hout = gadget_wires(consts, ww, l_in, r_in);
    if (out_wire < 0) ww.push(hout); else ww.put((uint32_t)out_wire, hout);
    if (h == 0) c = hout;
    if (h == 1) asset = hout;
    if (h != 3) cur = hout;
  }
}

// Boundary check of the claim records, one lane per field as k_check_transfer_records: every field canonical (< r), x < l (field 0),
// amount < 2^128 (field 1), the index inside the tree (field 5) -- compared on the integer words, not in the field.  bad[g] = lowest
// offending field of record g (the caller initialises it to 0xffffffff): 0 x, 1 amount, 2 token, 3 chain_id, 4 out_commitment,
// 5 index, 6 + l sibling l.
__global__ void __launch_bounds__(64) k_check_claim_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(C_REC + depth)) return;
  const uint8_t* rec = inputs + g * (size_t)(C_REC + depth) * 32;
  const uint8_t* p = rec + (size_t)f * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 0) {
    const uint32_t xw[8] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
    ok = ok && ed_below_order(xw);
  }
  if (f == 1) ok = ok && rec_amount_ok(w);
  if (f == 5) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void claim_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_claim_records, dim3(grid_for(C_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream, inputs_d, a.depth, n, bad_d);
}

// (claim_witness has asked for the table of BASE before records_witness gets here)
static void claim_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_claim_core, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, (const uint8_t*)ctx->ed_tab_d,
                     inputs_d, depth, (size_t)s.n_wires, (uint32_t)s.first_bit_wire, n, out_d);
}

// the 64 x 16 table of BASE is built on the context's stream by the first call that needs it (eddsa_keys.hip); then the walk of the
// record statements, which is lane-local for the owned statements (claim, send, redeem) whatever n
static int claim_witness(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  const uint8_t* tab = nullptr;
  OG_TRY(eddsa_base_table(ctx, &tab));
  return records_witness(st, ctx, a, inputs_d, n, out_d);
}

// ---- the send and the redeem statement: an owned note spent directly, as transfer and as split spend an ordinary one ---------------------
// Specs: tests/send_spec.py, tests/redeem_spec.py.  Both have claim's front -- x = sum 2^i b_i over 251 boolean wires, x < l, P = x BASE,
// c = H(P.x, P.y), asset = H(amount, token), leaf = H(c, asset) under root, nullifier_hash = H(x, 1): the SAME hash claim publishes, so
// the ledger's one spent set stops a note that was claimed from also being sent or redeemed -- without claim's one * one row, and then
//   send:    transfer's back.  public: root, nullifier_hash, chain_id, pay_leaf, change_leaf (n_pub = 5); pay_amount + change = amount
//            with both below 2^128, pay_leaf = H(pay_commitment, H(pay_amount, token)), change_leaf = H(change_commitment, H(change, token))
//   redeem:  split's back.  public: root, nullifier_hash, recipient, amount_out, token, chain_id, change_leaf (n_pub = 7); amount_out +
//            change = amount with both below 2^128, change_leaf = H(change_commitment, H(change, token))
// The commitments are unconstrained: an ordinary c' or the c of an owned or view note.  No reference counterpart.
// Input records, (8 + depth) x 32 B canonical LE:
//   send:    x | amount | token | chain_id | pay_commitment | pay_amount | change_commitment | index (u64 in the low bytes) | siblings[depth]
//   redeem:  x | amount | recipient | amount_out | token | chain_id | change_commitment | index | siblings[depth]
// Wires of send:
//   0 one | 1 root | 2 nullifier_hash | 3 chain_id | 4 pay_leaf | 5 change_leaf
//   6 x | 7 amount | 8 token | 9 pay_commitment | 10 pay_amount | 11 change_commitment | 12 change
//   13.. siblings[D] | index bits[D] | chain_id^2 | pay_amount bits[128] (LSB first) | change bits[128] | x bits[251] | the comparison's 114
//   wires | the multiplication's 5 x 251 wires (as in claim) | the gadgets: c, asset, leaf, nullifier_hash (out = wire 2), level 0..D-1
//   (the last one's out = wire 1), pay_asset, pay_leaf (out = wire 4), change_asset, change_leaf (out = wire 5)
// Wires of redeem:
//   0 one | 1 root | 2 nullifier_hash | 3 recipient | 4 amount_out | 5 token | 6 chain_id | 7 change_leaf
//   8 x | 9 amount | 10 change_commitment | 11 change
//   12.. siblings[D] | index bits[D] | recipient^2 | chain_id^2 | amount_out bits[128] | change bits[128] | x bits[251] | the comparison's
//   114 wires | the multiplication's wires | the gadgets: c, asset, leaf, nullifier_hash (out = wire 2), level 0..D-1 (the last one's
//   out = wire 1), change_asset, change_leaf (out = wire 7)
// One walk each, one lane per request: k_send_core, k_redeem_core.  The wires of the key are claim's, from owned_key_wires.  What the
// back of the walk needs of the record it loads where it needs it, as every walk loads its siblings, so that no more values live
// across the multiplication than in k_claim_core.  NOT built: a wave-wide walk, host chains.
constexpr int SN_PUB = 5, RD_PUB = 7;
constexpr int SN_REC = 8, RD_REC = 8;  // fields of a record before the siblings
constexpr int OW_RANGE = 128;          // bits of an amount
// byte offsets of the records' fields (x is field 0 of both, as of claim's: claim_x_bit)
constexpr int SN_X = 0, SN_AMOUNT = 32, SN_TOKEN = 64, SN_CHAIN = 96, SN_PAY_COMMITMENT = 128, SN_PAY_AMOUNT = 160, SN_CHANGE_COMMITMENT = 192,
              SN_INDEX = 224;
constexpr int RD_X = 0, RD_AMOUNT = 32, RD_RECIPIENT = 64, RD_AMOUNT_OUT = 96, RD_TOKEN = 128, RD_CHAIN = 160, RD_CHANGE_COMMITMENT = 192,
              RD_INDEX = 224;
static_assert(SN_X == C_X && RD_X == C_X, "claim_x_bit reads field 0");

// both shapes: `fields` wires before the siblings (one, the public and the private inputs), `squares` wires behind the index bits,
// `rows` rows before the range rows, `back` hashes behind the path, `pub_outs` of all hashes with a public output wire
static RecordShape owned_spend_shape(int depth, int fields, int squares, int rows, int back, int pub_outs) {
  RecordShape s{};
  const uint64_t hashes = 4 + (uint64_t)depth + back;
  s.first_bit_wire = fields + 2 * (uint64_t)depth + squares;  // the first range bit; the bits of x follow the 256 range bits
  s.first_gadget_wire = s.first_bit_wire + 2 * OW_RANGE + C_BITS + C_CMP + 5 * C_BITS;
  s.n_wires = s.first_gadget_wire + depth + hashes * 730 - pub_outs;  // a `left` per level
  s.n_constraints = rows + 2 * (OW_RANGE + 1) + 1 + C_BITS + 6 * C_BITS + 2 * (uint64_t)depth + hashes * 730;
  return s;
}
static RecordShape send_shape(const StatementArgs& a) { return owned_spend_shape(a.depth, 1 + SN_PUB + 7, 1, 2, 4, 4); }
static RecordShape redeem_shape(const StatementArgs& a) { return owned_spend_shape(a.depth, 1 + RD_PUB + 4, 2, 3, 2, 3); }

// change = amount - part (pay_amount, amount_out) on the record's integer words, as transfer_change: the records are checked first,
// part <= amount < 2^128, so the difference does not borrow.  transfer_bit_wire gives the 256 range bits.
__device__ __forceinline__ TransferChange owned_change(const uint8_t* in, int amount_off, int part_off) {
  const uint64_t a_lo = *reinterpret_cast<const uint64_t*>(in + amount_off), a_hi = *reinterpret_cast<const uint64_t*>(in + amount_off + 8);
  TransferChange c;
  c.p_lo = *reinterpret_cast<const uint64_t*>(in + part_off);
  c.p_hi = *reinterpret_cast<const uint64_t*>(in + part_off + 8);
  c.c_lo = a_lo - c.p_lo;
  c.c_hi = a_hi - c.p_hi - (a_lo < c.p_lo ? 1u : 0u);
  return c;
}
__device__ __forceinline__ Fr rec_field(const uint8_t* in, int off) { return fe_to_mont(fe_load<FrParams>(in + off)); }

__global__ void __launch_bounds__(64) k_send_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const uint8_t* __restrict__ inputs,
                                                 int depth, size_t n_wires, uint32_t first_bit_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(SN_REC + depth) * 32;
  uint8_t* z = out + g * n_wires * 32;
  WireWriterT<false> ww{z, first_bit_wire};
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + SN_INDEX);
  {
    const Fr chain_id = rec_field(in, SN_CHAIN);
    const TransferChange chg = owned_change(in, SN_AMOUNT, SN_PAY_AMOUNT);
    ww.put(0, Fr::one());
    ww.put(3, chain_id);
    ww.put(6, rec_field(in, SN_X));
    ww.put(7, rec_field(in, SN_AMOUNT));
    ww.put(8, rec_field(in, SN_TOKEN));
    ww.put(9, rec_field(in, SN_PAY_COMMITMENT));
    ww.put(10, rec_field(in, SN_PAY_AMOUNT));
    ww.put(11, rec_field(in, SN_CHANGE_COMMITMENT));
    ww.put(12, chg.value());
    for (int l = 0; l < depth; l++) {
      ww.put(13 + l, rec_field(in, (SN_REC + l) * 32));
      ww.put(13 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
    }
    ww.put(13 + 2 * depth, fe_sqr(chain_id));
#pragma unroll 1
    for (int i = 0; i < 2 * OW_RANGE; i++) ww.push(transfer_bit_wire(chg, i));  // the bits of pay_amount, then of change, LSB first
  }
  Fr px, py;  // P = x BASE, affine
  owned_key_wires(tab, in, z, ww, px, py);
  // gadget 0: c = H(P.x, P.y); 1: asset = H(amount, token); 2: leaf = H(c, asset); 3: nullifier_hash = H(x, 1) -> wire 2; 4 + l: level
  // l of the path (wire 1 = root for the last level); 4 + depth: pay_asset = H(pay_amount, token); 5 + depth: pay_leaf =
  // H(pay_commitment, pay_asset) -> wire 4; 6 + depth: change_asset = H(change, token); 7 + depth: change_leaf = H(change_commitment,
  // change_asset) -> wire 5
  const Fr token = rec_field(in, SN_TOKEN);
  Fr cur = Fr::zero(), c = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 8 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = px; r_in = py;
    } else if (h == 1) {
      l_in = rec_field(in, SN_AMOUNT); r_in = token;
    } else if (h == 2) {
      l_in = c; r_in = cur;
    } else if (h == 3) {
      l_in = rec_field(in, SN_X); r_in = Fr::one(); out_wire = 2;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = rec_field(in, (SN_REC + lvl) * 32);
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    } else if (h == 4 + depth) {
      l_in = rec_field(in, SN_PAY_AMOUNT); r_in = token;
    } else if (h == 5 + depth) {
      l_in = rec_field(in, SN_PAY_COMMITMENT); r_in = cur; out_wire = 4;
    } else if (h == 6 + depth) {
      l_in = owned_change(in, SN_AMOUNT, SN_PAY_AMOUNT).value(); r_in = token;
    } else {
      l_in = rec_field(in, SN_CHANGE_COMMITMENT); r_in = cur; out_wire = 5;
    }
    const Fr hout = gadget_wires(consts, ww, l_in, r_in);
    if (out_wire < 0) ww.push(hout); else ww.put((uint32_t)out_wire, hout);
    if (h == 0) c = hout;
    if (h != 3) cur = hout;
  }
}

__global__ void __launch_bounds__(64) k_redeem_core(const uint32_t* __restrict__ consts, const uint8_t* __restrict__ tab, const uint8_t* __restrict__ inputs,
                                                   int depth, size_t n_wires, uint32_t first_bit_wire, size_t n, uint8_t* __restrict__ out) {
  OG_FILLER_PRIO();
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* in = inputs + g * (size_t)(RD_REC + depth) * 32;
  uint8_t* z = out + g * n_wires * 32;
  WireWriterT<false> ww{z, first_bit_wire};
  const uint64_t index = *reinterpret_cast<const uint64_t*>(in + RD_INDEX);
  {
    const Fr recipient = rec_field(in, RD_RECIPIENT), chain_id = rec_field(in, RD_CHAIN);
    const TransferChange chg = owned_change(in, RD_AMOUNT, RD_AMOUNT_OUT);
    ww.put(0, Fr::one());
    ww.put(3, recipient);
    ww.put(4, rec_field(in, RD_AMOUNT_OUT));
    ww.put(5, rec_field(in, RD_TOKEN));
    ww.put(6, chain_id);
    ww.put(8, rec_field(in, RD_X));
    ww.put(9, rec_field(in, RD_AMOUNT));
    ww.put(10, rec_field(in, RD_CHANGE_COMMITMENT));
    ww.put(11, chg.value());
    for (int l = 0; l < depth; l++) {
      ww.put(12 + l, rec_field(in, (RD_REC + l) * 32));
      ww.put(12 + depth + l, ((index >> l) & 1) ? Fr::one() : Fr::zero());
    }
    ww.put(12 + 2 * depth, fe_sqr(recipient));
    ww.put(13 + 2 * depth, fe_sqr(chain_id));
#pragma unroll 1
    for (int i = 0; i < 2 * OW_RANGE; i++) ww.push(transfer_bit_wire(chg, i));  // the bits of amount_out, then of change, LSB first
  }
  Fr px, py;  // P = x BASE, affine
  owned_key_wires(tab, in, z, ww, px, py);
  // gadget 0: c = H(P.x, P.y); 1: asset = H(amount, token); 2: leaf = H(c, asset); 3: nullifier_hash = H(x, 1) -> wire 2; 4 + l: level
  // l of the path (wire 1 = root for the last level); 4 + depth: change_asset = H(change, token); 5 + depth: change_leaf =
  // H(change_commitment, change_asset) -> wire 7
  const Fr token = rec_field(in, RD_TOKEN);
  Fr cur = Fr::zero(), c = Fr::zero();
#pragma unroll 1
  for (int h = 0; h < 6 + depth; h++) {
    Fr l_in, r_in;
    int out_wire = -1;
    if (h == 0) {
      l_in = px; r_in = py;
    } else if (h == 1) {
      l_in = rec_field(in, RD_AMOUNT); r_in = token;
    } else if (h == 2) {
      l_in = c; r_in = cur;
    } else if (h == 3) {
      l_in = rec_field(in, RD_X); r_in = Fr::one(); out_wire = 2;
    } else if (h < 4 + depth) {
      const int lvl = h - 4;
      const Fr sib = rec_field(in, (RD_REC + lvl) * 32);
      const bool right_child = (index >> lvl) & 1;
      l_in = right_child ? sib : cur;
      r_in = right_child ? cur : sib;
      ww.push(l_in);  // the `left` selector wire
      if (lvl == depth - 1) out_wire = 1;
    } else if (h == 4 + depth) {
      l_in = owned_change(in, RD_AMOUNT, RD_AMOUNT_OUT).value(); r_in = token;
    } else {
      l_in = rec_field(in, RD_CHANGE_COMMITMENT); r_in = cur; out_wire = 7;
    }
    const Fr hout = gadget_wires(consts, ww, l_in, r_in);
    if (out_wire < 0) ww.push(hout); else ww.put((uint32_t)out_wire, hout);
    if (h == 0) c = hout;
    if (h != 3) cur = hout;
  }
}

// Boundary check of the send and of the redeem records, one lane per field as k_check_claim_records: every field canonical (< r),
// x < l (field 0), amount < 2^128 (field 1), the part that is paid below 2^128 and at most amount (field PART: 5 pay_amount in a send
// record, 3 amount_out in a redeem record), the index inside the tree (field 7) -- compared on the integer words, not in the field.
// bad[g] = lowest offending field of record g (the caller initialises it to 0xffffffff); 8 + l is sibling l.
template <int PART>
__global__ void __launch_bounds__(64) k_check_owned_spend_records(const uint8_t* __restrict__ inputs, int depth, size_t n, uint32_t* __restrict__ bad) {
  OG_FILLER_PRIO();
  static_assert(SN_REC == RD_REC && SN_AMOUNT == RD_AMOUNT && SN_INDEX == RD_INDEX, "one kernel text for both records");
  const size_t g = blockIdx.y;
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || f >= (uint32_t)(SN_REC + depth)) return;
  const uint8_t* rec = inputs + g * (size_t)(SN_REC + depth) * 32;
  const uint8_t* p = rec + (size_t)f * 32;
  bool ok = fe_lt_modulus(fe_load<FrParams>(p));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  if (f == 0) {
    const uint32_t xw[8] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
    ok = ok && ed_below_order(xw);
  }
  if (f == 1 || f == PART) ok = ok && rec_amount_ok(w);
  if (f == PART) ok = ok && rec_le(w, reinterpret_cast<const uint32_t*>(rec + SN_AMOUNT));  // the part <= amount
  if (f == SN_INDEX / 32) ok = ok && rec_index_ok(w, depth);
  if (!ok) atomicMin(&bad[g], f);
}

static void send_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_owned_spend_records<SN_PAY_AMOUNT / 32>, dim3(grid_for(SN_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream,
                     inputs_d, a.depth, n, bad_d);
}
static void redeem_launch_check(og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  hipLaunchKernelGGL(k_check_owned_spend_records<RD_AMOUNT_OUT / 32>, dim3(grid_for(RD_REC + a.depth, 64), (unsigned)n), dim3(64), 0, ctx->stream,
                     inputs_d, a.depth, n, bad_d);
}

// (claim_witness, which is their witness entry too, has asked for the table of BASE before records_witness gets here)
static void send_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_send_core, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, (const uint8_t*)ctx->ed_tab_d,
                     inputs_d, depth, (size_t)s.n_wires, (uint32_t)s.first_bit_wire, n, out_d);
}
static void redeem_launch_core(og_ctx* ctx, int depth, const RecordShape& s, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  hipLaunchKernelGGL(k_redeem_core, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, (const uint32_t*)ctx->mimc_consts_d, (const uint8_t*)ctx->ed_tab_d,
                     inputs_d, depth, (size_t)s.n_wires, (uint32_t)s.first_bit_wire, n, out_d);
}

// ---- the statements: one descriptor each, and the host code they share (statements.h) --------------------------------------------------
static const char* const WITHDRAW_FIELDS[W_REC] = {"nullifier", "secret", "amount", "recipient", "pad_seed", "index", "token", "chain_id"};
static const char* const DEPOSIT_FIELDS[D_REC] = {"nullifier", "secret", "depositor"};
static const char* const SPLIT_FIELDS[S_REC] = {"nullifier", "secret", "amount", "recipient", "amount_out", "index", "token", "chain_id", "change_commitment"};
static const char* const JOIN_FIELDS[J_REC] = {"nullifier_a", "secret_a", "amount_a", "index_a", "nullifier_b", "secret_b", "amount_b", "index_b",
                                               "token", "chain_id", "out_commitment"};
static const char* const TRANSFER_FIELDS[T_REC] = {"nullifier", "secret", "amount", "index", "token", "chain_id", "pay_commitment", "pay_amount",
                                                   "change_commitment"};
static const char* const CLAIM_FIELDS[C_REC] = {"x", "amount", "token", "chain_id", "out_commitment", "index"};
static const char* const SEND_FIELDS[SN_REC] = {"x", "amount", "token", "chain_id", "pay_commitment", "pay_amount", "change_commitment", "index"};
static const char* const REDEEM_FIELDS[RD_REC] = {"x", "amount", "recipient", "amount_out", "token", "chain_id", "change_commitment", "index"};
#define OG_RECORD_TAIL(what) "is not a valid value (>= r, an index outside the tree, an amount >= 2^128, " what ")"
#ifndef __HIP_DEVICE_COMPILE__  // (host data: the device pass would emit the tables too, and has none of the functions they name)
const Statement ST_WITHDRAW = {"withdraw", W_PUB, W_REC, 1, WITHDRAW_FIELDS, "is not a canonical value (>= r, or an index outside the tree)",
                               "this withdraw-circuit shape", withdraw_record_shape, withdraw_launch_check, withdraw_witness};
const Statement ST_DEPOSIT = {"deposit", D_PUB, D_REC, 0, DEPOSIT_FIELDS, "is not a canonical value (>= r)", "the deposit statement",
                              deposit_shape, deposit_launch_check, deposit_witness};
const Statement ST_SPLIT = {"split", S_PUB, S_REC, 1, SPLIT_FIELDS, OG_RECORD_TAIL("or amount_out > amount"), "this split-statement shape", split_shape,
                            split_launch_check, records_witness, SW9_XCH, split_launch_core, split_launch_w9, split_r1cs_rows};
const Statement ST_JOIN = {"join", J_PUB, J_REC, 2, JOIN_FIELDS, OG_RECORD_TAIL("amount_a + amount_b >= 2^128, or nullifier_b = nullifier_a"),
                           "this join-statement shape", join_shape, join_launch_check, records_witness, JW9_XCH, join_launch_core, join_launch_w9,
                           join_r1cs_rows};
const Statement ST_TRANSFER = {"transfer", T_PUB, T_REC, 1, TRANSFER_FIELDS, OG_RECORD_TAIL("or pay_amount > amount"), "this transfer-statement shape",
                               transfer_shape, transfer_launch_check, records_witness, TW9_XCH, transfer_launch_core, transfer_launch_w9,
                               transfer_r1cs_rows};
const Statement ST_CLAIM = {"claim", C_PUB, C_REC, 1, CLAIM_FIELDS, OG_RECORD_TAIL("or x >= l"), "this claim-statement shape", claim_shape,
                            claim_launch_check, claim_witness, 0, claim_launch_core, nullptr, claim_r1cs_rows};
const Statement ST_SEND = {"send", SN_PUB, SN_REC, 1, SEND_FIELDS, OG_RECORD_TAIL("x >= l, or pay_amount > amount"), "this send-statement shape",
                           send_shape, send_launch_check, claim_witness, 0, send_launch_core, nullptr, send_r1cs_rows};
const Statement ST_REDEEM = {"redeem", RD_PUB, RD_REC, 1, REDEEM_FIELDS, OG_RECORD_TAIL("x >= l, or amount_out > amount"), "this redeem-statement shape",
                             redeem_shape, redeem_launch_check, claim_witness, 0, redeem_launch_core, nullptr, redeem_r1cs_rows};
#endif

// the argument checks every call of a statement with a path makes (deposit has neither a depth nor a bound on its flat check grid)
static int statement_args_ok(const Statement& st, const StatementArgs& a) {
  OG_REQUIRE(st.paths == 0 || (a.depth >= 1 && a.depth <= 64), std::string(st.name) + ": depth must be 1..64");
  return OG_OK;
}

int records_shape_query(const Statement& st, const StatementArgs& a, uint64_t out[3]) {
  OG_TRY(statement_args_ok(st, a));
  const RecordShape s = st.shape(a);
  OG_REQUIRE(s.n_wires < (1ull << 31), std::string(st.name) + ": too many wires");  // (withdraw's padding alone can get there)
  out[0] = s.n_wires; out[1] = s.n_constraints; out[2] = (uint64_t)st.n_pub;
  return OG_OK;
}

int records_check_enqueue(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint32_t* bad_d) {
  OG_TRY(statement_args_ok(st, a));
  // (the record index is grid.y; checked HERE so that the caller gets this message, not a launch error)
  OG_REQUIRE(st.paths == 0 || n <= 65535, std::string(st.name) + ": at most 65535 records per call");
  if (n == 0) return OG_OK;
  st.launch_check(ctx, a, inputs_d, n, bad_d);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

// a sibling is named by its level, and with two paths by its path too: `sibling L`, or `sibling a L` / `sibling b L`
std::string invalid_record_message(const Statement& st, const std::string& who, int depth, size_t g, uint32_t f) {
  const uint32_t sib = f - (uint32_t)st.n_rec;
  const std::string name = f < (uint32_t)st.n_rec ? std::string(st.field_names[f])
                           : st.paths <= 1        ? "sibling " + std::to_string(sib)  // (no path: no division by a depth of 0)
                                                  : std::string("sibling ") + (char)('a' + sib / depth) + " " + std::to_string(sib % depth);
  return who + ": input record " + std::to_string(g) + ": field " + std::to_string(f) + " (" + name + ") " + st.invalid_tail;
}

int records_ok(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, size_t base) {
  if (n == 0) return OG_OK;  // (the witness entry that follows names a bad depth)
  uint32_t* bad_d = nullptr;
  OG_TRY(arena_get(ctx, "rec.bad", n * 4, (void**)&bad_d));
  OG_HIP(hipMemsetAsync(bad_d, 0xff, n * 4, ctx->stream));
  OG_TRY(records_check_enqueue(st, ctx, a, inputs_d, n, bad_d));
  std::vector<uint32_t> bad(n);
  OG_HIP(hipMemcpyAsync(bad.data(), bad_d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  OG_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t g = 0; g < n; g++)
    if (bad[g] != 0xffffffffu) {
      set_error(invalid_record_message(st, "og_" + std::string(st.name), a.depth, base + g, bad[g]));
      return OG_ERR_INVALID;
    }
  return OG_OK;
}

// The wave-wide walk for the calls witness_walks_wave_wide names -- its limb buffer is n x n_wires x 36 B from the arena --, the lane-local
// kernel for batches: there a wave per permutation would be paid out of the prover's accumulations.  A statement without a wave-wide
// form (claim, send, redeem) walks lane-local whatever n
int records_witness(const Statement& st, og_ctx* ctx, const StatementArgs& a, const uint8_t* inputs_d, size_t n, uint8_t* out_d) {
  OG_TRY(statement_args_ok(st, a));
  OG_REQUIRE(n <= 65535, std::string(st.name) + ": at most 65535 witnesses per call");
  if (n == 0) return OG_OK;
  const int depth = a.depth;
  const RecordShape s = st.shape(a);
  ProfScope ps(ctx, PROF_WITNESS, (double)n);
  if (st.launch_w9 && witness_walks_wave_wide(ctx, n)) {
    uint32_t *wl = nullptr, *xch = nullptr;
    OG_TRY(arena_get(ctx, "wit.w9.limbs", n * (size_t)s.n_wires * 36, (void**)&wl));
    OG_TRY(arena_get(ctx, "wit.w9.xch", n * (size_t)(st.paths * depth + st.w9_xch) * 36, (void**)&xch));
    st.launch_w9(ctx, depth, s, inputs_d, n, wl, xch);
    OG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_wires_from_limbs, dim3(grid_for(s.n_wires, 256), (unsigned)n), dim3(256), 0, ctx->stream, (const uint32_t*)wl, out_d,
                       (size_t)s.n_wires, (uint32_t)s.n_wires);
    OG_HIP(hipGetLastError());
    return OG_OK;
  }
  st.launch_core(ctx, depth, s, inputs_d, n, out_d);
  OG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_wires_from_mont, dim3(grid_for(s.n_wires, 256), (unsigned)n), dim3(256), 0, ctx->stream, out_d, (size_t)s.n_wires,
                     (uint32_t)s.n_wires, 1u);
  OG_HIP(hipGetLastError());
  return OG_OK;
}

}  // namespace og
