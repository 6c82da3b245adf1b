// ldpc_onchip.hpp -- host/device types of the on-chip decode path
// (ldpc_onchip.hip): one frame per workgroup, every message of the frame in
// the workgroup's LDS for the whole decode.
//
// For codes between the small-code kernel (one wave's registers, E <= 512)
// and the large-code kernels (messages in HBM): a few thousand edges, degrees
// up to the large-code limits.  H is the context's CSR / CSC (ldpc_graph.hpp)
// packed into 16-bit fields, which every code that fits the LDS also fits.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ldpc_graph.hpp"
#include "ldpc_kernels.hpp"
#include "ldpc_wglimits.hpp"

namespace ldpc {

constexpr int kOnchipLdsLimit = kWgLdsLimit;
constexpr int kOnchipMaxThreads = kWgMaxThreads;
constexpr int kOnchipIndexMax = kWgIndexMax;

// Byte offsets of one frame's state in the workgroup's dynamic LDS.
//   A     Real[E]  bit -> check: tanh(M/2) (sum-product) or L(q) (min-sum)
//   R     Real[E]  check -> bit
//   tab   the mode's log table (sum-product; stage_tab)
//   chan  float[N] -tx (widening to Real is exact)
//   hard  uint8[N] hard decisions
//   red   the workgroup's reduction words (ldpc_wglimits.hpp)
// and, where they fit behind the frame (`staged`), copies of the code's
// tables (OnchipTables), made once per workgroup; otherwise the kernels read
// the tables from global memory (L2) in every pass.
struct OnchipLayout {
  int r, tab, chan, hard, red;
  int erow, ecol, rows, cols, ci, ce;  // staged tables
  int staged;   // 1: the tables are in LDS
  int frame;    // bytes of the frame's state alone: what must fit
  int total;    // bytes the launch declares (frame, plus the tables when staged)
  int threads;  // multiple of 64, <= kOnchipMaxThreads
};

// The layout for a code and mode; true when it fits (degrees within
// kGraphDcMax / kGraphDvMax, indices within 16 bits, frame <= kOnchipLdsLimit).
// The layout is filled in either way.  Host only, no device needed.
bool onchip_plan(int M, int N, int E, int dc_max, int dv_max, int method, int prec,
                 OnchipLayout &L);

struct OnchipTables {
  std::vector<uint32_t> erow;  // E: row's first edge | degree << 16 | place in the row << 24
  std::vector<uint32_t> ecol;  // 2 E: {column | place in the column << 16, cols[column]}
  std::vector<uint32_t> rows;  // M: first edge | degree << 16
  std::vector<uint32_t> cols;  // N: offset into ce | degree << 16
  std::vector<uint16_t> ci;    // E: column of CSR edge e
  std::vector<uint16_t> ce;    // E: CSR edge ids, column by column, rows ascending
};
// From the context's CSR (rp, ci) and CSC (cp, ce) of build_graph.
void onchip_build(int M, int N, const std::vector<int32_t> &rp, const std::vector<int32_t> &ci,
                  const std::vector<int32_t> &cp, const std::vector<int32_t> &ce, OnchipTables &t);

struct OnchipView {
  const uint32_t *erow;
  const uint2 *ecol;
  const uint32_t *rows;
  const uint32_t *cols;
  const uint16_t *ci;
  const uint16_t *ce;
  int M, N, E, KB, dc_max, dv_max;
};

// Launches one decode (method 0 min-sum, 1 sum-product) of args.B frames on
// `stream`.  args.ticket / ticket_base / static_stride as in DecodeArgs
// (`waves` is set here: the resident workgroups).  *advance_out: what the
// launch adds to its counter.  resident[method][prec] caches the workgroups
// per CU of each kernel (0: not looked up yet).  Returns 0, -2 when the code
// does not fit, -3 on a launch error.
int launch_onchip_decode(const OnchipView &g, const DecodeArgs &args, int method, int prec,
                         void *stream, int (*resident)[4], uint32_t *advance_out);

}  // namespace ldpc
