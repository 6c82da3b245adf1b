// A stand-alone run of rate matching's host code (the C ABI's host entry points
// in ldpc_capi_host.cc over ldpc_rate_match.cc), for building with
// -fsanitize=address,undefined (make -C gr-ldpc_ece535a_amd rate_match_asan).
// Reads the cases tests/rate_match_cases.py writes -- "M N punct filler ncb
// n_tx B", the (k0, E) pairs, B rows of N bits, B rows of sum E floats as hex
// words -- and for each: plans it, checks every sample's column against the
// literal walk of the buffer, selects the bits of each transmission, recovers
// the samples from buffers of exactly the size the call states, and checks
// them against a sum taken sample by sample.  Then the refusals.  Exit status
// 0 iff all pass.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ldpc_capi_host.hpp"
#include "ldpc_hip.h"

// (ldpc_last_error is the context code's; this program links the host files alone)
static int fail(int c, const char *what) {
  fprintf(stderr, "case %d: %s (%s)\n", c, what, ldpc::capi::create_error().c_str());
  return 1;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int M, N, punct, filler, ncb, n_tx, B, cases = 0;
  while (fscanf(f, "%d %d %d %d %d %d %d", &M, &N, &punct, &filler, &ncb, &n_tx, &B) == 7) {
    std::vector<int32_t> k0((size_t)n_tx), e((size_t)n_tx);
    int64_t total = 0;
    for (int t = 0; t < n_tx; ++t) {
      if (fscanf(f, "%d %d", &k0[t], &e[t]) != 2) return 2;
      total += e[t];
    }
    std::vector<uint8_t> bits((size_t)B * N);
    std::string row((size_t)N + 1, '\0');
    for (int b = 0; b < B; ++b) {
      if (fscanf(f, "%s", &row[0]) != 1) return 2;
      for (int i = 0; i < N; ++i) bits[(size_t)b * N + i] = (uint8_t)(row[i] - '0');
    }
    std::vector<float> rx((size_t)B * total);
    for (auto &v : rx) {
      unsigned w;
      if (fscanf(f, "%x", &w) != 1) return 2;
      memcpy(&v, &w, 4);
    }
    std::vector<int32_t> col((size_t)total), count((size_t)N);
    if (ldpc_plan_rate_match(M, N, punct, filler, ncb, n_tx, k0.data(), e.data(), col.data(),
                             count.data()) != total)
      return fail(cases, "plan");
    // the literal walk
    const int K = N - M, nc = ncb ? ncb : N - punct;
    int64_t at = 0, sum = 0;
    for (int t = 0; t < n_tx; ++t)
      for (int j = k0[t], n = 0; n < e[t]; j = (j + 1) % nc) {
        const int pos = punct + j;
        if (pos >= K - filler && pos < K) continue;
        if (col[at++] != (pos < K ? M + pos : pos - K)) return fail(cases, "column");
        ++n;
      }
    for (int c = 0; c < N; ++c) {
      const int pos = c >= M ? c - M : c + K;
      const bool fill = pos >= K - filler && pos < K;
      if ((count[c] == -1) != fill) return fail(cases, "filler count");
      if (count[c] > 0 && (pos < punct || pos >= punct + nc)) return fail(cases, "unsent column");
      sum += count[c] > 0 ? count[c] : 0;
    }
    if (sum != total) return fail(cases, "counts");
    // bit selection, each transmission into a buffer of exactly B x E
    for (int t = 0; t < n_tx; ++t) {
      std::vector<uint8_t> out((size_t)B * e[t]);
      if (ldpc_rate_match(M, N, punct, filler, ncb, k0[t], e[t], bits.data(), B, out.data(),
                          e[t]) != LDPC_OK)
        return fail(cases, "rate_match");
      const int32_t *ct = col.data();
      int64_t off = 0;
      for (int s = 0; s < t; ++s) off += e[s];
      for (int b = 0; b < B; ++b)
        for (int i = 0; i < e[t]; ++i)
          if (out[(size_t)b * e[t] + i] != bits[(size_t)b * N + ct[off + i]])
            return fail(cases, "selected bit");
    }
    // the combine, at both polarities
    for (float pol : {1.0f, -1.0f}) {
      std::vector<float> y((size_t)B * N);
      const float un = 0x1p-100f;
      if (ldpc_rate_recover(M, N, punct, filler, ncb, rx.data(), (int64_t)rx.size(), total, pol,
                            un, B, n_tx, k0.data(), e.data(), y.data()) != LDPC_OK)
        return fail(cases, "rate_recover");
      for (int b = 0; b < B; ++b) {
        std::vector<float> want((size_t)N, un);
        std::vector<char> have((size_t)N, 0);
        for (int c = 0; c < N; ++c)
          if (count[c] == -1) want[c] = INFINITY;
        for (int64_t i = 0; i < total; ++i) {
          volatile float tx = rx[(size_t)b * total + i] * pol;
          const float v = -tx;
          want[col[i]] = have[col[i]] ? want[col[i]] + v : v;
          have[col[i]] = 1;
        }
        for (int c = 0; c < N; ++c) {
          const float w = -want[c], g = y[(size_t)b * N + c];
          if (memcmp(&w, &g, 4) != 0 && !(w != w && g != g)) return fail(cases, "recovered sample");
        }
      }
    }
    printf("case %d: M %d N %d pattern %d %d %d n_tx %d samples %lld ok\n", cases, M, N, punct,
           filler, ncb, n_tx, (long long)total);
    ++cases;
  }
  // the refusals, on a 4 x 12 code (K = 8)
  const int32_t k[1] = {0}, e1[1] = {4}, kbad[1] = {12}, ebig[1] = {16 * 12 + 1}, ezero[1] = {0};
  const int bad[][3] = {{-1, 0, 0}, {0, -1, 0}, {7, 2, 0}, {0, 0, 7}, {2, 0, 11}, {0, 8, 8}};
  for (const auto &p : bad)
    if (ldpc_plan_rate_match(4, 12, p[0], p[1], p[2], 1, k, e1, nullptr, nullptr) != LDPC_EINVAL)
      return fail(-1, "a bad pattern was accepted");
  if (ldpc_plan_rate_match(4, 12, 0, 0, 0, 1, kbad, e1, nullptr, nullptr) != LDPC_EINVAL ||
      ldpc_plan_rate_match(4, 12, 0, 0, 0, 1, k, ebig, nullptr, nullptr) != LDPC_EINVAL ||
      ldpc_plan_rate_match(4, 12, 0, 0, 0, 1, k, ezero, nullptr, nullptr) != LDPC_EINVAL ||
      ldpc_plan_rate_match(4, 12, 0, 0, 0, 0, k, e1, nullptr, nullptr) != LDPC_EINVAL ||
      ldpc_plan_rate_match(4, 12, 0, 0, 0, 5, k, e1, nullptr, nullptr) != LDPC_EINVAL)
    return fail(-1, "a bad transmission was accepted");
  float one[4] = {1, 1, 1, 1}, out[12];
  if (ldpc_rate_recover(4, 12, 0, 0, 0, one, 4, 4, 1.0f, NAN, 1, 1, k, e1, out) != LDPC_EINVAL ||
      ldpc_rate_recover(4, 12, 0, 0, 0, one, 4, 3, 1.0f, 0.0f, 1, 1, k, e1, out) != LDPC_EINVAL ||
      ldpc_rate_recover(4, 12, 0, 0, 0, one, 3, 4, 1.0f, 0.0f, 1, 1, k, e1, out) != LDPC_EINVAL)
    return fail(-1, "a bad combine was accepted");
  return cases > 0 ? 0 : 2;
}
