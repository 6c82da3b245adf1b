// ldpc_capi_host.cc -- the part of the C ABI (include/ldpc_hip.h) that needs no
// device: H ingestion (the constructor's matrix + reorderHMatrix,
// lib/ldpc_decoder_cb_impl.cc:60-106), the alist parser, the reference
// encoder, the GF(2) recognisers the device encoder is prepared with, rate
// matching's host forms (ldpc_rate_match.hpp) and the code-block CRC's
// (ldpc_crc.hpp).  Integer and GF(2) arithmetic,
// and the combine's float adds; built by the host compiler.
#include "ldpc_capi_host.hpp"

#include <stdio.h>

#include <algorithm>

#include "../../include/ldpc_hip.h"
#include "ldpc_crc.hpp"
#include "ldpc_rate_match.hpp"

namespace ldpc {
namespace capi {

namespace {
thread_local std::string g_create_error;
}  // namespace

int set_create_error(int code, const std::string &msg) {
  g_create_error = msg;
  return code;
}

void clear_create_error() { g_create_error.clear(); }

const std::string &create_error() { return g_create_error; }

// reorderHMatrix, lib/ldpc_decoder_cb_impl.cc:255-307 ('First' strategy):
// for each row i pick the first column j >= i with F(i,j) != 0 (column 0 if
// none), swap columns i and j of F and H, and clear column i below row i
// with GF(2) row additions.  lower/upper (M x (N-M), optional) receive the
// factors the encoder solves with (lib/ldpc_encoder_bc_impl.cc:259-260).
void reorder_columns(uint8_t *H, int M, int N, int32_t *chosen, std::vector<uint8_t> *lower,
                     std::vector<uint8_t> *upper) {
  std::vector<uint8_t> F(H, H + (size_t)M * N);
  const int K = N - M;
  if (lower) lower->assign((size_t)M * std::max(K, 0), 0);
  if (upper) upper->assign((size_t)M * std::max(K, 0), 0);
  for (int i = 0; i < M; ++i) {
    int pick = 0;
    for (int j = i; j < N; ++j)
      if (F[(size_t)i * N + j]) {
        pick = j;
        break;
      }
    if (chosen) chosen[i] = pick;
    if (pick != i)
      for (int r = 0; r < M; ++r) {
        std::swap(F[(size_t)r * N + i], F[(size_t)r * N + pick]);
        std::swap(H[(size_t)r * N + i], H[(size_t)r * N + pick]);
      }
    if (i < K) {
      if (lower)
        for (int r = i; r < M; ++r) (*lower)[(size_t)r * K + i] = F[(size_t)r * N + i];
      if (upper)
        for (int r = 0; r <= i; ++r) (*upper)[(size_t)r * K + i] = F[(size_t)r * N + i];
    }
    for (int k = i + 1; k < M; ++k)
      if (F[(size_t)k * N + i])
        for (int c = 0; c < N; ++c) F[(size_t)k * N + c] ^= F[(size_t)i * N + c];
  }
}

bool valid_h(const uint8_t *H, int M, int N) {
  if (!H || M <= 0 || N <= 0 || M >= N) return false;
  for (size_t t = 0; t < (size_t)M * N; ++t)
    if (H[t] > 1) return false;
  return true;
}

void dense_to_csr(const uint8_t *H, int M, int N, std::vector<int32_t> &rp,
                  std::vector<int32_t> &ci) {
  rp.assign((size_t)M + 1, 0);
  ci.clear();
  for (int j = 0; j < M; ++j) {
    for (int i = 0; i < N; ++i)
      if (H[(size_t)j * N + i]) ci.push_back(i);
    rp[j + 1] = (int32_t)ci.size();
  }
}

bool valid_csr(int M, int N, const int32_t *rp, const int32_t *ci) {
  if (!rp || M <= 0 || N <= 0 || M >= N || rp[0] != 0) return false;
  for (int j = 0; j < M; ++j) {
    if (rp[j + 1] < rp[j]) return false;
    for (int32_t e = rp[j]; e < rp[j + 1]; ++e) {
      if (!ci || ci[e] < 0 || ci[e] >= N) return false;
      if (e > rp[j] && ci[e] <= ci[e - 1]) return false;  // ascending, no duplicates
    }
  }
  return true;
}

bool systematic_matrix(const uint8_t *H, int M, int N, std::vector<uint64_t> &A) {
  const int K = N - M, W = (N + 63) / 64;
  std::vector<uint64_t> rows((size_t)M * W, 0);
  for (int j = 0; j < M; ++j)
    for (int i = 0; i < N; ++i)
      if (H[(size_t)j * N + i]) rows[(size_t)j * W + i / 64] |= 1ull << (i % 64);
  for (int c = 0; c < M; ++c) {
    int piv = -1;
    for (int r = c; r < M; ++r)
      if ((rows[(size_t)r * W + c / 64] >> (c % 64)) & 1) {
        piv = r;
        break;
      }
    if (piv < 0) return false;
    if (piv != c)
      for (int w = 0; w < W; ++w) std::swap(rows[(size_t)piv * W + w], rows[(size_t)c * W + w]);
    for (int r = 0; r < M; ++r)
      if (r != c && ((rows[(size_t)r * W + c / 64] >> (c % 64)) & 1))
        for (int w = 0; w < W; ++w) rows[(size_t)r * W + w] ^= rows[(size_t)c * W + w];
  }
  const int KW = (K + 63) / 64;
  A.assign((size_t)M * KW, 0);
  for (int j = 0; j < M; ++j)
    for (int i = 0; i < K; ++i)
      if ((rows[(size_t)j * W + (M + i) / 64] >> ((M + i) % 64)) & 1)
        A[(size_t)j * KW + i / 64] |= 1ull << (i % 64);
  return true;
}

bool has_staircase(int M, const int32_t *rp, const int32_t *ci) {
  for (int j = 0; j < M; ++j) {
    int want[2] = {j - 1, j}, n = 0;
    bool ok = true;
    for (int32_t e = rp[j]; e < rp[j + 1] && ci[e] < M; ++e) {
      const int c = ci[e];
      if (n >= 2 || (j == 0 ? c != 0 : c != want[n])) ok = false;
      ++n;
    }
    if (!ok || n != (j == 0 ? 1 : 2)) return false;
  }
  return true;
}

namespace {

// The reference decoder's H, lib/ldpc_decoder_cb_impl.cc:63-96 (32 x 64),
// one 64-bit word per row, bit c = column c.
const uint64_t kDefaultH[32] = {
    0x0000504000000140ull, 0x0000024080100020ull, 0x0020000141004000ull,
    0x000a008000000220ull, 0x0000080400848000ull, 0x0008000401000090ull,
    0x4100400204000000ull, 0x0010301000000001ull, 0x00024c0000000008ull,
    0x9500006000000000ull, 0x0101200080000400ull, 0x1040000000002004ull,
    0x3080080002000002ull, 0x0200800008010010ull, 0x0410018008040000ull,
    0x0000001200005020ull, 0x0080000040802200ull, 0x0020008010480000ull,
    0x0400001000018088ull, 0x2002020000200004ull, 0x0000000300080300ull,
    0xc200000000240080ull, 0x02000000e4000000ull, 0x0800000000301002ull,
    0x2000040008402040ull, 0x8800010400080000ull, 0x0070000000800000ull,
    0x4040010800000840ull, 0x000c02000000c800ull, 0x0000002811000008ull,
    0x0884000010000401ull, 0x0000900902020000ull,
};

int alist_err(const std::string &msg) { return set_create_error(LDPC_EINVAL, msg); }

}  // namespace
}  // namespace capi
}  // namespace ldpc

using namespace ldpc::capi;

extern "C" {

int ldpc_default_h(uint8_t *H_out) {
  if (!H_out) return LDPC_EINVAL;
  for (int j = 0; j < 32; ++j)
    for (int i = 0; i < 64; ++i) H_out[j * 64 + i] = (uint8_t)((kDefaultH[j] >> i) & 1);
  return LDPC_OK;
}

// MacKay's alist format: "N M", "max_col_deg max_row_deg", the N column
// degrees, the M row degrees, then per column its rows and per row its
// columns (1-based), each list zero-padded to the maximum degree or not
// padded at all (both forms are in use).  The row lists must agree with the
// column lists.
int ldpc_alist_read(const char *path, int *M_out, int *N_out, int32_t *row_ptr_opt,
                    int32_t *col_idx_opt, int64_t col_idx_cap) {
  if (!path || !M_out || !N_out) return alist_err("null argument");
  FILE *f = fopen(path, "r");
  if (!f) return alist_err(std::string("cannot open ") + path);
  std::vector<long> v;
  long x;
  while (fscanf(f, "%ld", &x) == 1) v.push_back(x);
  const bool clean_eof = feof(f) != 0;
  fclose(f);
  if (!clean_eof) return alist_err("alist: non-numeric content");
  if (v.size() < 4) return alist_err("alist: truncated header");
  const long N = v[0], M = v[1], dvm = v[2], dcm = v[3];
  if (N <= 0 || M <= 0 || M >= N || N > (1L << 24) || dvm <= 0 || dcm <= 0 ||
      v.size() < (size_t)(4 + N + M))
    return alist_err("alist: bad header (need 0 < M < N)");
  long sum_c = 0, sum_r = 0;
  for (long i = 0; i < N; ++i) {
    const long d = v[4 + i];
    if (d < 0 || d > dvm) return alist_err("alist: bad column degree");
    sum_c += d;
  }
  for (long j = 0; j < M; ++j) {
    const long d = v[4 + N + j];
    if (d < 0 || d > dcm) return alist_err("alist: bad row degree");
    sum_r += d;
  }
  if (sum_c != sum_r) return alist_err("alist: degree sums differ");
  const size_t head = 4 + N + M;
  bool padded;
  // (the header's maximum degrees are unbounded in the unpadded form: a product
  // that overflows is no length a file can have)
  long pad_c, pad_r, pad;
  if (!__builtin_mul_overflow(N, dvm, &pad_c) && !__builtin_mul_overflow(M, dcm, &pad_r) &&
      !__builtin_add_overflow(pad_c, pad_r, &pad) && v.size() == head + (size_t)pad)
    padded = true;
  else if (v.size() == head + (size_t)(sum_c + sum_r))
    padded = false;
  else
    return alist_err("alist: list length matches neither padded nor unpadded");
  // column lists -> (row, col) pairs; row lists checked against them
  std::vector<std::vector<int32_t>> rows(M);
  size_t at = head;
  for (long i = 0; i < N; ++i) {
    const long d = v[4 + i], width = padded ? dvm : d;
    for (long k = 0; k < width; ++k) {
      const long r = v[at++];
      if (k >= d) {
        if (r != 0) return alist_err("alist: non-zero padding");
        continue;
      }
      if (r < 1 || r > M) return alist_err("alist: row index out of range");
      rows[r - 1].push_back((int32_t)i);
    }
  }
  int64_t E = 0;
  for (long j = 0; j < M; ++j) {
    std::vector<int32_t> &c = rows[j];
    std::sort(c.begin(), c.end());
    if (std::adjacent_find(c.begin(), c.end()) != c.end()) return alist_err("alist: repeated entry");
    const long d = v[4 + N + j], width = padded ? dcm : d;
    if ((long)c.size() != d) return alist_err("alist: row degree mismatch");
    std::vector<int32_t> listed;
    for (long k = 0; k < width; ++k) {
      const long cc = v[at++];
      if (k >= d) {
        if (cc != 0) return alist_err("alist: non-zero padding");
        continue;
      }
      if (cc < 1 || cc > N) return alist_err("alist: column index out of range");
      listed.push_back((int32_t)(cc - 1));
    }
    std::sort(listed.begin(), listed.end());
    if (listed != c) return alist_err("alist: row and column lists disagree");
    E += d;
  }
  *M_out = (int)M;
  *N_out = (int)N;
  if (row_ptr_opt) {
    row_ptr_opt[0] = 0;
    for (long j = 0; j < M; ++j) row_ptr_opt[j + 1] = row_ptr_opt[j] + (int32_t)rows[j].size();
  }
  if (col_idx_opt) {
    if (col_idx_cap < E) return alist_err("alist: col_idx buffer too small");
    int64_t o = 0;
    for (long j = 0; j < M; ++j)
      for (int32_t c : rows[j]) col_idx_opt[o++] = c;
  }
  return (int)E;
}

int ldpc_reorder_h(uint8_t *H, int M, int N, int32_t *chosen_opt) {
  if (!valid_h(H, M, N)) return LDPC_EINVAL;
  reorder_columns(H, M, N, chosen_opt, nullptr, nullptr);
  return LDPC_OK;
}

int ldpc_check_frame(const uint8_t *H, int M, int N, const uint8_t *bits, int threshold) {
  if (!valid_h(H, M, N) || !bits) return LDPC_EINVAL;
  int unsatisfied = 0;
  for (int k = 0; k < M; ++k) {
    int parity = 0;
    for (int j = 0; j < N; ++j) parity ^= (H[(size_t)k * N + j] & (bits[j] & 1));
    if (parity) ++unsatisfied;
    if (unsatisfied > threshold) break;
  }
  return unsatisfied;
}

// makeParityCheck (lib/ldpc_encoder_bc_impl.cc:275-294) over GF(2): the
// reference's two real-valued dgesv solves on the unit-triangular 0/1
// factors are exact integer substitutions, which reduce mod 2 to the
// substitutions below.  The factors come from re-running the reorder on the
// (already reordered) H, which then moves no column.
int ldpc_encode(const uint8_t *Hr, int M, int N, const uint8_t *data_bits, int B,
                uint8_t *codewords_out) {
  if (!valid_h(Hr, M, N) || N != 2 * M || B < 0 || (B > 0 && (!data_bits || !codewords_out)))
    return LDPC_EINVAL;
  std::vector<uint8_t> H(Hr, Hr + (size_t)M * N), L, U;
  std::vector<int32_t> chosen(M);
  reorder_columns(H.data(), M, N, chosen.data(), &L, &U);
  for (int i = 0; i < M; ++i)
    if (chosen[i] != i) return LDPC_EINVAL;  // not the reordered form
  const int K = N - M;
  for (int i = 0; i < M; ++i)
    if (!L[(size_t)i * K + i] || !U[(size_t)i * K + i]) return LDPC_ESINGULAR;
  std::vector<uint8_t> z(M), x(M);
  for (int b = 0; b < B; ++b) {
    const uint8_t *d = data_bits + (size_t)b * K;
    uint8_t *cw = codewords_out + (size_t)b * N;
    for (int i = 0; i < M; ++i) {
      int acc = 0;
      for (int j = 0; j < K; ++j) acc ^= Hr[(size_t)i * N + M + j] & (d[j] & 1);
      z[i] = (uint8_t)acc;
    }
    for (int i = 0; i < M; ++i) {  // L x = z
      int acc = z[i];
      for (int j = 0; j < i; ++j) acc ^= L[(size_t)i * K + j] & x[j];
      x[i] = (uint8_t)acc;
    }
    for (int i = M - 1; i >= 0; --i) {  // U c = x
      int acc = x[i];
      for (int j = i + 1; j < M; ++j) acc ^= U[(size_t)i * K + j] & cw[j];
      cw[i] = (uint8_t)acc;
    }
    for (int j = 0; j < K; ++j) cw[M + j] = d[j] & 1;
  }
  return LDPC_OK;
}

// Rate matching on the host (ldpc_rate_match.hpp): the plan of a call, the bit
// selection and the soft combine, by the index functions the kernels run.
int64_t ldpc_plan_rate_match(int M, int N, int punct, int filler, int ncb, int n_tx,
                             const int32_t *k0, const int32_t *e, int32_t *col_out_opt,
                             int32_t *count_out_opt) {
  clear_create_error();
  ldpc::RmArgs rm;
  std::string why;
  if (!ldpc::rm_pattern(M, N, punct, filler, ncb, rm, &why))
    return set_create_error(LDPC_EINVAL, "bad rate-matching pattern: " + why);
  const int64_t total = ldpc::rm_transmissions(rm, n_tx, k0, e, &why);
  if (total < 0) return set_create_error(LDPC_EINVAL, "bad transmission: " + why);
  ldpc::rm_plan(rm, col_out_opt, count_out_opt);
  return total;
}

int ldpc_rate_match(int M, int N, int punct, int filler, int ncb, int k0, int E,
                    const uint8_t *bits, int B, uint8_t *out, int64_t out_stride) {
  clear_create_error();
  ldpc::RmArgs rm;
  std::string why;
  if (!ldpc::rm_pattern(M, N, punct, filler, ncb, rm, &why))
    return set_create_error(LDPC_EINVAL, "bad rate-matching pattern: " + why);
  const int32_t k0s[1] = {k0}, es[1] = {E};
  if (ldpc::rm_transmissions(rm, 1, k0s, es, &why) < 0)
    return set_create_error(LDPC_EINVAL, "bad transmission: " + why);
  if (B < 0 || out_stride < E || (B > 0 && (!bits || !out)))
    return set_create_error(LDPC_EINVAL, "bad arguments: B >= 0, out_stride >= E, buffers given");
  ldpc::rm_match(rm, bits, B, out, out_stride);
  return LDPC_OK;
}

int ldpc_rate_recover(int M, int N, int punct, int filler, int ncb, const float *rx,
                      int64_t n_rx_floats, int64_t rx_stride, float polarity,
                      float unreceived_lci, int B, int n_tx, const int32_t *k0, const int32_t *e,
                      float *samples_out) {
  clear_create_error();
  ldpc::RmArgs rm;
  std::string why;
  if (!ldpc::rm_pattern(M, N, punct, filler, ncb, rm, &why))
    return set_create_error(LDPC_EINVAL, "bad rate-matching pattern: " + why);
  const int64_t total = ldpc::rm_transmissions(rm, n_tx, k0, e, &why);
  if (total < 0) return set_create_error(LDPC_EINVAL, "bad transmission: " + why);
  if (unreceived_lci != unreceived_lci)
    return set_create_error(LDPC_EINVAL, "unreceived_lci must not be NaN");
  if (B < 0 || rx_stride < total || (B > 0 && (!rx || !samples_out)))
    return set_create_error(LDPC_EINVAL,
                            "bad arguments: B >= 0, rx_stride >= the sum of E, buffers given");
  if (B > 0 && (int64_t)(B - 1) * rx_stride + total > n_rx_floats)
    return set_create_error(LDPC_EINVAL, "input shorter than the frames read");
  rm.unreceived = unreceived_lci;
  ldpc::rm_recover(rm, rx, rx_stride, polarity, B, samples_out);
  return LDPC_OK;
}

// The code-block CRC on the host (ldpc_crc.hpp): the register, the block and
// its weights, and the attach, by the text ldpc_set_crc builds its table with.
int64_t ldpc_crc_bits(int len, uint32_t poly, const uint8_t *bits, int64_t n) {
  clear_create_error();
  std::string why;
  if (!ldpc::crc_check(len, poly, &why)) return set_create_error(LDPC_EINVAL, "bad CRC: " + why);
  if (n < 0 || (n > 0 && !bits))
    return set_create_error(LDPC_EINVAL, "bad arguments: n >= 0, bits given");
  return (int64_t)ldpc::crc_bits(len, poly, bits, n);
}

int ldpc_plan_crc(int M, int N, int filler, int len, uint32_t poly, uint32_t *weights_out_opt) {
  clear_create_error();
  std::string why;
  if (!ldpc::crc_check(len, poly, &why)) return set_create_error(LDPC_EINVAL, "bad CRC: " + why);
  const int A = ldpc::crc_block(M, N, filler, len, &why);
  if (A < 0) return set_create_error(LDPC_EINVAL, "bad CRC: " + why);
  if (weights_out_opt) ldpc::crc_weights(len, poly, A, weights_out_opt);
  return A;
}

int ldpc_crc_attach(int M, int N, int filler, int len, uint32_t poly, const uint8_t *payload,
                    int B, uint8_t *info_out) {
  clear_create_error();
  std::string why;
  if (!ldpc::crc_check(len, poly, &why)) return set_create_error(LDPC_EINVAL, "bad CRC: " + why);
  const int A = ldpc::crc_block(M, N, filler, len, &why);
  if (A < 0) return set_create_error(LDPC_EINVAL, "bad CRC: " + why);
  if (B < 0 || (B > 0 && (!payload || !info_out)))
    return set_create_error(LDPC_EINVAL, "bad arguments: B >= 0, buffers given");
  ldpc::crc_attach(len, poly, A, N - M, payload, B, info_out);
  return LDPC_OK;
}

}  // extern "C"
