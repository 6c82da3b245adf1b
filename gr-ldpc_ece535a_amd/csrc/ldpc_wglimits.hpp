// ldpc_wglimits.hpp -- limits and LDS bookkeeping of the workgroup-per-frame
// kernels (ldpc_wgframe.hpp: the on-chip flooding kernels of ldpc_onchip.hip
// and the layered kernels of ldpc_layered.hip), for their planners and for
// the device header.  No HIP header: it is usable from files the host compiler
// builds, such as ldpc_layers.cc.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace ldpc {

constexpr int kWgLdsLimit = 160 * 1024;  // LDS a workgroup may declare on MI355X
constexpr int kWgMaxThreads = 1024;
constexpr int kWgIndexMax = 65535;       // M, N, E: the tables' 16-bit fields

// The `red` region every frame layout ends with, in 32-bit words:
//   [0, 16)  per-wave counts (wg_sum_waves), one word per wave of the workgroup
//   [16]     the workgroup's next frame (wg_next_frame)
//   [17, 29) the code-block CRC's per-wave remainders, three bytes per wave
//            (ldpc_layered.hip crc_wave_share: sixteen 24-bit values do not
//            fit fifteen words one apiece)
//   [29, 32) unused
constexpr int kWgRedWaves = 16, kWgRedNext = 16, kWgRedWords = 32;
constexpr int kWgRedCrc = 17, kWgRedCrcWords = 12;
static_assert(kWgRedWaves * 3 == kWgRedCrcWords * 4 && kWgRedCrc + kWgRedCrcWords <= kWgRedWords,
              "three bytes per wave of the largest workgroup");
constexpr int kWgRedBytes = kWgRedWords * 4;
static_assert(kWgMaxThreads / 64 <= kWgRedWaves, "a count word per wave of the largest workgroup");

constexpr int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// Carves a workgroup's dynamic LDS into regions of 16-byte-aligned sizes, in
// the order they are taken.  Offsets saturate at INT_MAX: a layout is filled in
// for any code, and one that does not fit is refused by its size, never by an
// offset that wrapped.
struct LdsCarve {
  int64_t end = 0;  // bytes taken so far
  static int sat(int64_t x) { return (int)std::min<int64_t>(x, 0x7fffffff); }
  int take(int64_t bytes) {
    const int64_t at = end;
    end += a16(bytes);
    return sat(at);
  }
};

}  // namespace ldpc
