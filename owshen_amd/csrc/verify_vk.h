// What og_vk_load computes on the host from the key alone (verify_vk.hip: vk_precompute, which reuses og_verify's own decoding,
// Miller loop and affine step) and hands to the kernels of verify_gpu.hip.  Internal; not part of the C ABI.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../include/owshen_gpu.h"  // og_ctx, og_vk

namespace og {

// steps of the optimal-ate twist walk: 64 doublings, one addition per set bit below the leading one of 6x + 2 (36), two Frobenius steps
constexpr size_t VK_WALK_STEPS = 64 + 36 + 2;
// device constants, 64 B (one Fq2, Montgomery) each
enum { VK_C_HALF = 0, VK_C_BT = 1, VK_C_G12 = 2, VK_C_G13 = 3, VK_C_G22 = 4, VK_C_G23 = 5, VK_C_FROB = 6, VK_N_CONSTS = 24 };

struct VkHost {
  uint64_t n_pub = 0;
  std::vector<uint32_t> ab;     // Miller value of (alpha, beta): coefficient k of w^k, component c, limb j at (2 k + c) * 9 + j
  std::vector<uint8_t> walk;    // gamma's walk, then delta's: per step slope | intercept (lambda x_T - y_T), 2 x 64 B Montgomery
  std::vector<uint8_t> ic;      // (n_pub + 1) x 64 B affine Montgomery; (0, 0) = the point at infinity
  std::vector<uint8_t> consts;  // VK_N_CONSTS x 64 B
};

int vk_precompute(const uint8_t* vk, size_t vk_len, VkHost& out);
// og_verify's own final exponentiation (the plain 2790-bit power) on a value in VkHost::ab's layout: is the result one?
bool f12_plain_is_one(const uint32_t limbs[108]);

// ---- the verifier's functions behind the entry points (capi.hip, verify_only.cpp) --------------------------------------------------
// og_verify on the CPU (verify.hip); the verifying key's layout: key_blob.h
int verify_cpu(const uint8_t* vk, size_t vk_len, const uint8_t* pub, size_t n_pub, const uint8_t* proof, int* ok);
// the og_vk handle and batched verification on the GPU (verify_gpu.hip)
int vk_load(og_ctx* ctx, const uint8_t* blob, size_t len, og_vk** out);
void vk_destroy(og_vk* vk);
void vk_info(const og_vk* vk, uint64_t info[4]);
int verify_batch(og_ctx* ctx, const og_vk* vk, const uint8_t* pub_d, const uint8_t* proofs_d, size_t n, uint32_t* ok_out);

}  // namespace og
