// What key generation from toxic waste (keygen.hip: og_setup) and from a powers-of-tau file (ptau.hip: og_setup_ptau) share:
// the QAP rows of a circuit, their transpose, the generators, and the one serialiser of the "OWPK0001" / "OWVK0001" blobs.
#pragma once
#include "ctx.h"
#include <string>
#include <vector>

namespace og {

extern const uint8_t G1_GEN_BYTES[64];    // canonical, x | y
extern const uint8_t G2_GEN_BYTES[128];   // the EIP-197 generator: x.c0 | x.c1 | y.c0 | y.c1

struct QapRows {  // constraints, then the n_pub + 1 input-consistency rows; CSR, canonical values
  std::vector<uint32_t> ptr[3], col[3];
  std::vector<uint8_t> val[3];
};
int r1cs_qap_rows(const og_r1cs* r, const std::string& who, QapRows* out);
void csr_transpose(const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& col, const std::vector<uint8_t>& val, size_t n_rows, size_t m,
                   std::vector<uint32_t>& tptr, std::vector<uint32_t>& tcol, std::vector<uint8_t>& tval);

struct KeyParts {  // canonical affine bytes on the host
  size_t m = 0, l = 0, n_rows = 0;
  int log_d = 0;
  const uint8_t *alpha1 = nullptr, *beta1 = nullptr, *delta1 = nullptr, *beta2 = nullptr, *gamma2 = nullptr, *delta2 = nullptr;
  const uint8_t* query[5] = {};  // A (m) | B in G1 (m) | B in G2 (m) | L (m - l - 1) | H (2^log_d - 1)
  const uint8_t* ic = nullptr;   // l + 1
};
void key_blobs(const KeyParts& k, const QapRows& rows, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk);

}  // namespace og
