// ldpc_rate_match.cc -- the host side of rate matching (ldpc_rate_match.hpp):
// the checks of a pattern and of a call's transmissions, the plan, and the
// host bit selection and soft combine, which run the index functions the
// kernels run.  Integer arithmetic and float adds; built by the host compiler.
#include "ldpc_rate_match.hpp"

#include <limits.h>

#include <algorithm>

namespace ldpc {

namespace {

bool refuse(std::string *why, const char *what, long long value) {
  if (why) *why = std::string(what) + " (got " + std::to_string(value) + ")";
  return false;
}

// tx = in * polarity, then Lci = -tx, as an operation of its own (the kernels'
// lci_term_of): folded into one multiply, or into a subtraction by the add that
// takes it, a NaN would keep the sign the negation flips.
inline float lci_of(float in, float polarity) {
  volatile float tx = in * polarity;
  volatile float v = -tx;
  return v;
}

}  // namespace

bool rm_pattern(int M, int N, int punct, int filler, int ncb, RmArgs &rm, std::string *why) {
  const int K = N - M;
  if (M <= 0 || K <= 0) return refuse(why, "rate matching needs 0 < M < N; N", N);
  if (punct < 0) return refuse(why, "punct must be >= 0", punct);
  if (filler < 0) return refuse(why, "filler must be >= 0", filler);
  if (ncb < 0) return refuse(why, "ncb must be >= 0 (0: N - punct)", ncb);
  if ((int64_t)punct + filler > K)
    return refuse(why, ("punct must be <= K - filler = " + std::to_string(K - filler)).c_str(),
                  punct);
  if (ncb == 0) ncb = N - punct;
  if ((int64_t)punct + ncb < K || (int64_t)punct + ncb > N)
    return refuse(why,
                  ("punct + ncb must be in [K, N] = [" + std::to_string(K) + ", " +
                   std::to_string(N) + "]; ncb")
                      .c_str(),
                  ncb);
  if (ncb - filler < 1) return refuse(why, "S = ncb - filler must be >= 1; S", ncb - filler);
  if ((int64_t)(ncb - filler) * kRmMaxRepeat * kRmMaxTx > INT_MAX)
    return refuse(why, "the buffer is too long for 32-bit sample indices; S", ncb - filler);
  rm = RmArgs{};  // the words of transmissions a call does not have stay 0
  rm.punct = punct;
  rm.filler = filler;
  rm.fs = K - filler - punct;
  rm.S = ncb - filler;
  rm.M = M;
  rm.K = K;
  return true;
}

int64_t rm_transmissions(RmArgs &rm, int n_tx, const int32_t *k0, const int32_t *e,
                         std::string *why) {
  if (n_tx < 1 || n_tx > kRmMaxTx || !k0 || !e) {
    refuse(why, "n_tx must be in [1, 4], with k0 and e given; n_tx", n_tx);
    return -1;
  }
  const int ncb = rm.S + rm.filler;
  int64_t total = 0;
  for (int t = 0; t < n_tx; ++t) {
    if (k0[t] < 0 || k0[t] >= ncb) {
      refuse(why, ("k0 must be in [0, ncb = " + std::to_string(ncb) + ")").c_str(), k0[t]);
      return -1;
    }
    if (e[t] < 1 || e[t] > (int64_t)kRmMaxRepeat * rm.S) {
      refuse(why, ("E must be in [1, 16 S = " + std::to_string((int64_t)kRmMaxRepeat * rm.S) + "]")
                      .c_str(),
             e[t]);
      return -1;
    }
    rm.u0[t] = rm_u0(rm.fs, rm.filler, rm.S, k0[t]);
    rm.E[t] = e[t];
    rm.off[t] = (int)total;
    total += e[t];
  }
  rm.n_tx = n_tx;
  return total;
}

void rm_plan(const RmArgs &rm, int32_t *col_out, int32_t *count_out) {
  const int N = rm.M + rm.K;
  if (count_out)
    for (int c = 0; c < N; ++c) count_out[c] = rm_u_of_col(rm, c) == kRmFiller ? -1 : 0;
  for (int t = 0; t < rm.n_tx; ++t)
    for (int e = 0; e < rm.E[t]; ++e) {
      const int c = rm_col_of_sample(rm, rm.u0[t], e);
      if (col_out) col_out[rm.off[t] + e] = c;
      if (count_out) ++count_out[c];
    }
}

void rm_match(const RmArgs &rm, const uint8_t *bits, int B, uint8_t *out, int64_t out_stride) {
  const int N = rm.M + rm.K;
  for (int b = 0; b < B; ++b)
    for (int e = 0; e < rm.E[0]; ++e)
      out[b * out_stride + e] = bits[(int64_t)b * N + rm_col_of_sample(rm, rm.u0[0], e)] & 1;
}

void rm_recover(const RmArgs &rm, const float *rx, int64_t rx_stride, float polarity, int B,
                float *samples) {
  const int N = rm.M + rm.K;
  for (int b = 0; b < B; ++b) {
    const float *src = rx + b * rx_stride;
    for (int c = 0; c < N; ++c)
      samples[(int64_t)b * N + c] =
          -rm_column_lci(rm, c, [&](int i) { return lci_of(src[i], polarity); });
  }
}

}  // namespace ldpc
