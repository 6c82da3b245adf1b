// ldpc_capi_host.hpp -- the C ABI's pure host code (ldpc_capi_host.cc): H
// ingestion and checks, the reference encoder's GF(2) algebra, and the
// creation-time error string.  No HIP, no ldpc_ctx: the file builds with the
// host compiler alone (make capi_host_asan runs it under the sanitizers).
// Private to the library: nothing here is exported.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace ldpc {
namespace capi {

// The error of calls that have no context (ldpc_create*, ldpc_plan_*, ...),
// per thread; ldpc_last_error(NULL) reads it.  set_create_error returns code.
int set_create_error(int code, const std::string &msg);
void clear_create_error();
const std::string &create_error();

// reorderHMatrix ('First' strategy) on a dense H, in place; lower / upper
// (M x (N-M), optional) receive the factors the encoder solves with.
void reorder_columns(uint8_t *H, int M, int N, int32_t *chosen, std::vector<uint8_t> *lower,
                     std::vector<uint8_t> *upper);
bool valid_h(const uint8_t *H, int M, int N);
bool valid_csr(int M, int N, const int32_t *rp, const int32_t *ci);
// CSR of a dense H (edges row-major, ascending column).
void dense_to_csr(const uint8_t *H, int M, int N, std::vector<int32_t> &rp,
                  std::vector<int32_t> &ci);

// Systematic encoder matrix of a dense H (codeword = [parity (M) | data (K)]):
// A = H_p^-1 H_d by Gauss-Jordan over GF(2), M rows of (K + 63) / 64 words,
// bit i of row j = A(j, i).  false: the first M columns of H are dependent.
bool systematic_matrix(const uint8_t *H, int M, int N, std::vector<uint64_t> &A);
// Whether columns 0..M-1 of a CSR H are the accumulator staircase (IRA /
// DVB-S2): row 0 has column 0 alone, row j columns j-1 and j.
bool has_staircase(int M, const int32_t *rp, const int32_t *ci);

}  // namespace capi
}  // namespace ldpc
#pragma GCC visibility pop
