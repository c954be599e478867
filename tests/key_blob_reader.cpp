// TEST INFRASTRUCTURE ONLY: owshen_amd/csrc/key_blob.h as a program of its own, for a sanitizer build (test_emu_key_blob.py).
// Reads a proving key from the file named on the command line, places it at byte offsets 0 .. 7 of a heap buffer sized to the
// byte, and at each offset parses it (pk_view), checks all three matrices (pk_csr_check) and sums every word the view leads
// to.  With -fsanitize=address,undefined a misaligned load or a read past the end of the blob ends the program.
#include "key_blob.h"
#include <stdio.h>
#include <stdlib.h>

namespace og {
void set_error(const std::string& msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}  // namespace og

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> key;
  for (int c; (c = fgetc(f)) != EOF;) key.push_back((uint8_t)c);
  fclose(f);
  uint64_t first = 0;
  for (size_t shift = 0; shift < 8; shift++) {
    uint8_t* buf = static_cast<uint8_t*>(malloc(key.size() + shift));  // (no slack behind the blob: one byte too far is a finding)
    memcpy(buf + shift, key.data(), key.size());
    og::PkView v;
    if (og::pk_view(buf + shift, key.size(), "reader", &v) != OG_OK || og::pk_csr_check(v, 3, "reader") != OG_OK) return 1;
    uint64_t sum = v.m + v.l + v.log_d + v.n_rows + v.flags + v.word9;
    for (int k = 0; k < 3; k++) {
      for (size_t r = 0; r <= v.n_rows; r++) sum += og::rd32(v.ptr[k] + r * 4);
      for (size_t i = 0; i < v.nnz[k]; i++) sum += og::rd32(v.col[k] + i * 4) + og::rd64(v.val[k] + i * 32 + 24);
    }
    for (int q = 0; q < 5; q++) sum += og::all_zero(v.query[q], v.q_bytes[q]) ? 1 : 0;
    if (v.off(v.query[4]) + og::pad32(v.q_bytes[4]) != key.size()) return 1;
    if (shift == 0) first = sum;
    if (sum != first) return 1;
    free(buf);
  }
  printf("ok 8 offsets\n");
  return 0;
}
