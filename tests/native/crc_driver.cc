// A stand-alone run of the code-block CRC's host code (the C ABI's host entry
// points in ldpc_capi_host.cc over ldpc_crc.cc), for building with
// -fsanitize=address,undefined (make -C gr-ldpc_ece535a_amd crc_asan).  Takes
// no input: the six known answers; then, for every named CRC and block lengths
// that include A = len + 1, A no multiple of 32 and A > 8192, seeded blocks in
// buffers of exactly the size each call states -- the weights' XOR against the
// register, the attach, the zero remainder of an attached block and the
// non-zero one of every single-bit error.  Then the refusals.  Exit status 0
// iff all pass.
#include <stdio.h>

#include <string>
#include <vector>

#include "ldpc_capi_host.hpp"
#include "ldpc_hip.h"

namespace {

struct Named {
  const char *name;
  int len;
  uint32_t poly, check;
};
const Named kCrcs[] = {{"CRC24A", LDPC_CRC24A_LEN, LDPC_CRC24A_POLY, 0xCDE703u},
                       {"CRC24B", LDPC_CRC24B_LEN, LDPC_CRC24B_POLY, 0x23EF52u},
                       {"CRC24C", LDPC_CRC24C_LEN, LDPC_CRC24C_POLY, 0xF48279u},
                       {"CRC16", LDPC_CRC16_LEN, LDPC_CRC16_POLY, 0x31C3u},
                       {"CRC11", LDPC_CRC11_LEN, LDPC_CRC11_POLY, 0x5CAu},
                       {"CRC6", LDPC_CRC6_LEN, LDPC_CRC6_POLY, 0x15u}};

// (ldpc_last_error is the context code's; this program links the host files alone)
int fail(const char *name, int A, const char *what) {
  fprintf(stderr, "%s A %d: %s (%s)\n", name, A, what, ldpc::capi::create_error().c_str());
  return 1;
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_bit() {  // xorshift64*: seeded, the same blocks every run
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 63);
}

uint32_t weights_xor(const std::vector<uint32_t> &w, const uint8_t *bits, int n) {
  uint32_t x = 0;
  for (int p = 0; p < n; ++p)
    if (bits[p] & 1) x ^= w[p];
  return x;
}

}  // namespace

int main() {
  std::vector<uint8_t> msg;
  for (const char *s = "123456789"; *s; ++s)
    for (int j = 7; j >= 0; --j) msg.push_back((uint8_t)((*s >> j) & 1));
  for (const Named &c : kCrcs)
    if (ldpc_crc_bits(c.len, c.poly, msg.data(), (int64_t)msg.size()) != (int64_t)c.check)
      return fail(c.name, 72, "known answer");

  int blocks = 0;
  for (const Named &c : kCrcs) {
    for (int A : {c.len + 1, c.len + 2, 33, 95, 284, 1000, 8193 + c.len}) {
      if (A <= c.len) continue;
      for (int filler : {0, 5}) {
        const int M = 7, K = A + filler, N = M + K, P = A - c.len, B = 3;
        std::vector<uint32_t> w((size_t)A);
        if (ldpc_plan_crc(M, N, filler, c.len, c.poly, w.data()) != A) return fail(c.name, A, "plan");
        if (w[(size_t)A - 1] != 1u) return fail(c.name, A, "the last weight is x^0");
        std::vector<uint8_t> payload((size_t)B * P), info((size_t)B * K, 0xff);
        for (auto &v : payload) v = (uint8_t)next_bit();
        if (ldpc_crc_attach(M, N, filler, c.len, c.poly, payload.data(), B, info.data()) != LDPC_OK)
          return fail(c.name, A, "attach");
        for (int b = 0; b < B; ++b, ++blocks) {
          const uint8_t *pl = payload.data() + (size_t)b * P;
          uint8_t *blk = info.data() + (size_t)b * K;
          const uint32_t reg = (uint32_t)ldpc_crc_bits(c.len, c.poly, pl, P);
          // the CRC field is the payload's register, and the XOR of its weights
          uint32_t field = 0;
          for (int j = 0; j < c.len; ++j) field = field << 1 | blk[P + j];
          if (field != reg || weights_xor(w, pl, P) != reg) return fail(c.name, A, "CRC field");
          for (int p = 0; p < P; ++p)
            if (blk[p] != pl[p]) return fail(c.name, A, "payload copy");
          for (int p = A; p < K; ++p)
            if (blk[p] != 0) return fail(c.name, A, "filler");
          if (weights_xor(w, blk, A) != 0) return fail(c.name, A, "an attached block passes");
          // every single-bit error (a sample of them on the long blocks)
          for (int p = 0; p < A; p += A > 2000 ? 97 : 1) {
            blk[p] ^= 1;
            const uint32_t rem = weights_xor(w, blk, A);
            uint32_t got = 0;
            for (int j = 0; j < c.len; ++j) got = got << 1 | blk[P + j];
            if (rem == 0 || rem != ((uint32_t)ldpc_crc_bits(c.len, c.poly, blk, P) ^ got))
              return fail(c.name, A, "a single-bit error");
            blk[p] ^= 1;
          }
        }
      }
    }
  }
  // the refusals
  uint8_t one[32] = {0}, out[32];
  if (ldpc_crc_bits(0, 0, one, 8) != LDPC_EINVAL || ldpc_crc_bits(25, 1, one, 8) != LDPC_EINVAL ||
      ldpc_crc_bits(6, 0x40, one, 8) != LDPC_EINVAL || ldpc_crc_bits(6, 0x21, nullptr, 8) != LDPC_EINVAL ||
      ldpc_crc_bits(6, 0x21, one, -1) != LDPC_EINVAL)
    return fail("refusals", 0, "a bad register call was accepted");
  if (ldpc_plan_crc(4, 12, 2, 6, 0x21, nullptr) != LDPC_EINVAL ||   // A = 6 = len
      ldpc_plan_crc(4, 12, 0, 16, 0x1021, nullptr) != LDPC_EINVAL ||  // A = 8 < len
      ldpc_plan_crc(4, 12, 0, 6, 0x21, nullptr) != 8 ||
      ldpc_crc_attach(4, 12, 2, 6, 0x21, one, 1, out) != LDPC_EINVAL ||
      ldpc_crc_attach(4, 12, 0, 6, 0x21, nullptr, 1, out) != LDPC_EINVAL ||
      ldpc_crc_attach(4, 12, 0, 6, 0x21, one, -1, out) != LDPC_EINVAL)
    return fail("refusals", 0, "a bad block was accepted");
  printf("crc: 6 known answers, %d blocks, refusals ok\n", blocks);
  return 0;
}
