// ldpc_layers.hpp -- the layer plan, LDS budget and tables of the layered
// min-sum decoder (ldpc_layered.hip).  Host only, no device needed.
//
// A layered (row-serial) decoder updates the posteriors row by row; rows that
// share no column may run side by side.  A plan assigns every row of H to one
// layer 0..L-1 such that no two rows of a layer share a column; the kernel
// runs the layers in order with one workgroup barrier between them, a thread
// per row of the current layer.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "ldpc_wglimits.hpp"

namespace ldpc {

constexpr int kLayeredLdsLimit = kWgLdsLimit;
constexpr int kLayeredMaxThreads = kWgMaxThreads;
constexpr int kLayeredIndexMax = kWgIndexMax;
constexpr int kLayeredDcMax = 32;

// First fit over the rows in ascending order: row j goes to the lowest layer
// with which it shares no column.  Deterministic; L >= the largest column
// degree.  layer_of_row gets M entries; returns L.
int plan_layers(int M, int N, const int32_t *rp, const int32_t *ci,
                std::vector<int32_t> &layer_of_row);

// Checks a caller's plan: every layer index in [0, M), no column twice in a
// layer.  Returns L (the largest index + 1), or -1 with the reason in *why
// (the two rows and the column of a collision).
int check_layers(int M, int N, const int32_t *rp, const int32_t *ci, const int32_t *layer_of_row,
                 std::string *why);

// Byte offsets of one frame's state in the workgroup's dynamic LDS:
//   LQ    Real[N]  posteriors L(Q_i), at offset 0
//   R     Real[E]  check -> bit messages
//   hard  uint8[N] hard decisions
//   red   the workgroup's reduction words (ldpc_wglimits.hpp)
// and, where they fit behind the frame (`staged`), copies of the code's
// tables (LayeredTables); otherwise the kernel reads them from global memory
// (L2).  E + N reals per frame, where the flooding on-chip path needs 2 E.
struct LayeredLayout {
  int r, hard, red;
  int rows, ci, order, off;  // staged tables
  int staged;   // 1: the tables are in LDS
  int frame;    // bytes of the frame's state alone: what must fit
  int total;    // bytes the launch declares (frame, plus the tables when staged)
  int threads;  // the largest layer's rows rounded up to 64, <= kLayeredMaxThreads
};

// The layout for a code, a plan (L layers, the largest of max_layer_rows rows)
// and a precision (1: float, else double); true when the code fits (dc_max <=
// kLayeredDcMax, indices within 16 bits, frame <= kLayeredLdsLimit).  Filled in
// either way.
bool layered_layout(int M, int N, int E, int dc_max, int L, int max_layer_rows, int prec,
                    LayeredLayout &lay);

// The fixed-point decoder's layout (ldpc_layered.hip Q8Arith): LQ int16[N] at
// offset 0, R int8[E] at `r`, the reduction words at `red` (`hard` is unused
// and equals `red`: the decisions are LQ < 0, read in place), every term
// rounded up to 16 bytes:
//   frame = a16(2 N) + a16(E) + 128
// Z == 0: the per-edge table route, whose 16-bit fields need E <=
// kLayeredIndexMax and whose tables are staged behind the frame where they
// fit; Z > 0: the circulant route at that lifting size, which stages nothing
// and whose words bound the base entries, E / Z <= kLayeredIndexMax, and E by
// the frame alone.  Either way M, N <= kLayeredIndexMax, dc_max <= kLayeredDcMax and
// 127 (dv_max + 1) <= 32767: LQ[c] = Lc_c + the sum of the column's R after
// every update, so |LQ| <= 127 (dv + 1) and int16 is exact without saturation.
constexpr int kLayeredQ8DvMax = 32767 / 127 - 1;
bool layered_q8_layout(int M, int N, int64_t E, int dc_max, int dv_max, int L,
                       int max_layer_rows, int Z, LayeredLayout &lay);

struct LayeredTables {
  std::vector<uint32_t> rows;   // M: first edge | degree << 16
  std::vector<uint16_t> ci;     // E: column of CSR edge e
  std::vector<uint16_t> order;  // M: the rows sorted by layer (stable: ascending row within one)
  std::vector<uint32_t> off;    // L + 1: layer l is order[off[l] .. off[l + 1])
  int L = 0;
};
void layered_build(int M, const int32_t *rp, const int32_t *ci,
                   const std::vector<int32_t> &layer_of_row, int L, LayeredTables &t);

}  // namespace ldpc
