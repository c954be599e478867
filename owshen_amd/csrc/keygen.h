// What key generation from toxic waste (keygen.hip: og_setup) and from a powers-of-tau file (ptau.hip: og_setup_ptau) share:
// the QAP rows of a circuit (QapRows: key_blob.h, beside the blobs' one serialiser, which takes them), their transpose, the generators.
#pragma once
#include "ctx.h"
#include "key_blob.h"
#include <string>
#include <vector>

namespace og {

extern const uint8_t G1_GEN_BYTES[64];    // canonical, x | y
extern const uint8_t G2_GEN_BYTES[128];   // the EIP-197 generator: x.c0 | x.c1 | y.c0 | y.c1

int r1cs_qap_rows(const og_r1cs* r, const std::string& who, QapRows* out);
void csr_transpose(const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& col, const std::vector<uint8_t>& val, size_t n_rows, size_t m,
                   std::vector<uint32_t>& tptr, std::vector<uint32_t>& tcol, std::vector<uint8_t>& tval);

}  // namespace og
