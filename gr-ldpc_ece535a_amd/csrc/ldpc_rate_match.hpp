// ldpc_rate_match.hpp -- rate matching (include/ldpc_hip.h):
// which codeword column a transmitted sample belongs to, and which samples a
// column is recovered from.  Integer arithmetic and one float add; the index
// functions are the same text for the host (ldpc_rate_match.cc, built by the
// host compiler: no HIP header here) and for the kernels (ldpc_aux.hip,
// ldpc_layered.hip).
//
// Transmit position p in [0, N) is column M + p for p < K (systematic first)
// and column p - K otherwise.  A pattern (punct, filler, ncb): positions
// [0, punct) are never sent, positions [K - filler, K) are known zeros and
// never sent, and the circular buffer is positions [punct, punct + ncb).  With
// the fillers taken out the buffer has S = ncb - filler compact indices u:
//   offset j = u < fs ? u : u + filler      fs = K - filler - punct
//   position = punct + j
// A transmission (k0, E) is the compact indices (u0 + e) mod S, e < E, where
//   u0 = (k0 < fs ? k0 : max(k0, fe) - filler) mod S      fe = K - punct
#pragma once

#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
// (the attributes spelled out: this header may come before the HIP runtime's)
#define LDPC_RM_FN \
  __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define LDPC_RM_FN inline
#endif

namespace ldpc {

constexpr int kRmMaxTx = 4;       // transmissions a call combines (LDPC_RM_MAX_TX)
constexpr int kRmMaxRepeat = 16;  // E <= 16 S

// A pattern and the transmissions of one call, resolved: what the kernels take
// by value.  off[t]: the first sample of transmission t within a frame's
// received samples (the sum of the E before it).
struct RmArgs {
  int punct, fs, filler, S, M, K;
  int n_tx;
  int u0[kRmMaxTx], E[kRmMaxTx], off[kRmMaxTx];
  float unreceived;  // the Lci of a column no sample reaches
};

LDPC_RM_FN int rm_col_of_pos(int M, int K, int p) { return p < K ? M + p : p - K; }
LDPC_RM_FN int rm_pos_of_col(int M, int K, int c) { return c >= M ? c - M : c + K; }

// The first compact index of a transmission that starts at buffer offset k0
// (0 <= k0 < S + filler): a k0 inside the fillers starts behind them.
LDPC_RM_FN int rm_u0(int fs, int filler, int S, int k0) {
  const int fe = fs + filler;
  const int u = k0 < fs ? k0 : (k0 > fe ? k0 : fe) - filler;  // <= S
  return u >= S ? u - S : u;
}

// Position of compact index u (0 <= u < S).
LDPC_RM_FN int rm_pos_of_u(const RmArgs &rm, int u) {
  return rm.punct + (u < rm.fs ? u : u + rm.filler);
}

// Column of sample e of a transmission that starts at u0.
LDPC_RM_FN int rm_col_of_sample(const RmArgs &rm, int u0, int e) {
  return rm_col_of_pos(rm.M, rm.K, rm_pos_of_u(rm, (int)(((int64_t)u0 + e) % rm.S)));
}

enum { kRmFiller = -1, kRmUnsent = -2 };

// Compact index of column c; kRmFiller for a filler column, kRmUnsent for a
// punctured column or one outside the buffer.
LDPC_RM_FN int rm_u_of_col(const RmArgs &rm, int c) {
  const int j = rm_pos_of_col(rm.M, rm.K, c) - rm.punct;
  if (j >= rm.fs && j < rm.fs + rm.filler) return kRmFiller;
  if (j < 0 || j >= rm.S + rm.filler) return kRmUnsent;
  return j < rm.fs ? j : j - rm.filler;
}

// The first sample of a transmission from u0 that lands on compact index u;
// the later ones follow in steps of S.  Both operands are below S: no division.
LDPC_RM_FN int rm_first_sample(int u, int u0, int S) {
  const int e = u - u0;
  return e < 0 ? e + S : e;
}

// Column c's Lci: its terms with transmissions ascending and, within one, e
// ascending; the first as it is, every later one a float add.  lci(i): the Lci
// of received sample i of the frame.  +inf for a filler, rm.unreceived where no
// sample lands.  A gather: no two columns share a term.
template <typename Lci>
LDPC_RM_FN float rm_column_lci(const RmArgs &rm, int c, const Lci &lci) {
  const int u = rm_u_of_col(rm, c);
  if (u == kRmFiller) return __builtin_inff();
  float acc = rm.unreceived;
  if (u < 0) return acc;
  bool have = false;
  for (int t = 0; t < rm.n_tx; ++t)
    for (int e = rm_first_sample(u, rm.u0[t], rm.S); e < rm.E[t]; e += rm.S) {
      const float v = lci(rm.off[t] + e);
      acc = have ? acc + v : v;
      have = true;
    }
  return acc;
}

// ---- host (ldpc_rate_match.cc) ---------------------------------------------------

// Checks a pattern on an M x N code and fills rm's pattern fields (n_tx = 0).
// False with *why naming the offending value.
bool rm_pattern(int M, int N, int punct, int filler, int ncb, RmArgs &rm, std::string *why);
// Checks the transmissions of a call against rm's pattern and fills n_tx, u0,
// E, off.  Returns the samples per frame (the sum of E), or -1 with *why.
int64_t rm_transmissions(RmArgs &rm, int n_tx, const int32_t *k0, const int32_t *e,
                         std::string *why);
// col_out (sum of E, optional): the column of every sample; count_out (N,
// optional): the samples that reach each column, -1 for a filler.
void rm_plan(const RmArgs &rm, int32_t *col_out, int32_t *count_out);
// Bit selection of transmission 0: bits (B, N) -> out (B, E) at out_stride.
void rm_match(const RmArgs &rm, const uint8_t *bits, int B, uint8_t *out, int64_t out_stride);
// The combine: rx (B frames at rx_stride) -> samples (B, N), y = -Lci.
void rm_recover(const RmArgs &rm, const float *rx, int64_t rx_stride, float polarity, int B,
                float *samples);

}  // namespace ldpc
