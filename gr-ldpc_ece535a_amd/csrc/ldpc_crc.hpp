// ldpc_crc.hpp -- the code-block CRC (include/ldpc_hip.h):
// the shift register, the per-position weights every kernel checks and
// attaches with, and the argument check.  Integer arithmetic; one text for the
// host (ldpc_crc.cc, built by the host compiler: no HIP header here) and the
// argument the kernels take by value (ldpc_layered.hip, ldpc_aux.hip).
//
// A CRC is (len, poly), 1 <= len <= 24, poly the generator g without its
// leading term.  Register 0 at the start, bits enter MSB first, no reflection,
// no final xor: the register over bits b_0 .. b_{n-1} ends as
//   (b_0 x^(n-1) + ... + b_{n-1}) x^len  mod g.
// The block is the A = K - filler information positions [0, A) in transmit
// order (position p is column M + p): payload [0, A - len), then the payload's
// register, MSB first.  Position p weighs w[p] = x^(A-1-p) mod g, so
//   the CRC field of a payload = XOR of w[p] over its one bits (p < A - len),
//   a block's remainder        = XOR of w[p] over its one bits (p < A)
//                              = register(payload) ^ the CRC field read MSB first,
// and 0 means pass.
#pragma once

#include <stdint.h>

#include <string>

namespace ldpc {

constexpr int kCrcMaxLen = 24;

enum { kCrcReport = 0, kCrcStop = 1 };

// What a kernel takes by value: the weights of the A block positions (device
// memory, read-only during a launch), the first information column M, whether
// a zero remainder ends a frame, and where frame b's remainder goes (out[b]).
struct CrcArgs {
  const uint32_t *w;
  int A, M;
  int stop;
  uint32_t *out;
};

// One step of the register: v * x mod g for v < 2^len.
inline uint32_t crc_times_x(int len, uint32_t poly, uint32_t v) {
  const uint32_t top = (v >> (len - 1)) & 1u;
  return ((v << 1) & ((1u << len) - 1u)) ^ (poly & (0u - top));
}

// ---- host (ldpc_crc.cc) ----------------------------------------------------------

// 1 <= len <= 24 and poly < 2^len; false with *why naming the offending value.
bool crc_check(int len, int64_t poly, std::string *why);
// The register over bit 0 of each of n bytes.
uint32_t crc_bits(int len, uint32_t poly, const uint8_t *bits, int64_t n);
// The block length A = (N - M) - filler of a checked CRC on an M x N code, or
// -1 with *why: A > len is required.
int crc_block(int M, int N, int filler, int len, std::string *why);
// w[p] = x^(A-1-p) mod g, p < A.
void crc_weights(int len, uint32_t poly, int A, uint32_t *w);
// payload (B, A - len) bytes -> info (B, K) bytes: payload, CRC MSB first,
// K - A zero fillers (bit 0 of each source byte).
void crc_attach(int len, uint32_t poly, int A, int K, const uint8_t *payload, int B,
                uint8_t *info);

}  // namespace ldpc
