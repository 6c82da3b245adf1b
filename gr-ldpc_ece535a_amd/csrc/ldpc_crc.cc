// ldpc_crc.cc -- the code-block CRC on the host (ldpc_crc.hpp): the bitwise
// shift register, the per-position weights and the argument check that the C
// ABI's host entry points (ldpc_capi_host.cc) and ldpc_set_crc share.
#include "ldpc_crc.hpp"

namespace ldpc {

bool crc_check(int len, int64_t poly, std::string *why) {
  if (len < 1 || len > kCrcMaxLen) {
    if (why) *why = "len must be in [1, 24] (got " + std::to_string(len) + ")";
    return false;
  }
  if (poly < 0 || poly >= ((int64_t)1 << len)) {
    if (why)
      *why = "poly must be below 2^len = " + std::to_string((int64_t)1 << len) + " (got " +
             std::to_string(poly) + ")";
    return false;
  }
  return true;
}

uint32_t crc_bits(int len, uint32_t poly, const uint8_t *bits, int64_t n) {
  uint32_t r = 0;
  for (int64_t i = 0; i < n; ++i)
    r = crc_times_x(len, poly, r ^ ((uint32_t)(bits[i] & 1) << (len - 1)));
  return r;
}

int crc_block(int M, int N, int filler, int len, std::string *why) {
  const int64_t A = (int64_t)N - M - filler;
  if (M < 0 || N < M || filler < 0 || A <= len) {
    if (why)
      *why = "the block must be longer than the CRC: A = K - filler = " + std::to_string(A) +
             ", len = " + std::to_string(len);
    return -1;
  }
  return (int)A;
}

void crc_weights(int len, uint32_t poly, int A, uint32_t *w) {
  // x^0 = 1 is below 2^len for every len >= 1
  uint32_t v = 1u;
  for (int p = A - 1; p >= 0; --p) {
    w[p] = v;
    v = crc_times_x(len, poly, v);
  }
}

void crc_attach(int len, uint32_t poly, int A, int K, const uint8_t *payload, int B,
                uint8_t *info) {
  const int P = A - len;
  for (int b = 0; b < B; ++b) {
    const uint8_t *src = payload + (int64_t)b * P;
    uint8_t *dst = info + (int64_t)b * K;
    for (int p = 0; p < P; ++p) dst[p] = src[p] & 1;
    const uint32_t r = crc_bits(len, poly, src, P);
    for (int j = 0; j < len; ++j) dst[P + j] = (uint8_t)((r >> (len - 1 - j)) & 1u);
    for (int p = A; p < K; ++p) dst[p] = 0;
  }
}

}  // namespace ldpc
