// ldpc_layered.hpp -- host/device types of the layered normalized min-sum
// decoders (ldpc_layered.hip): one frame per persistent workgroup, the frame's
// posteriors and check messages in LDS, the rows of H taken layer by layer
// (ldpc_layers.hpp).  A decode is an arithmetic (LayeredArith: double, float,
// or int8 messages with int16 posteriors) on a route: per-edge tables for any
// plan (LayeredView), or the base matrix of a quasi-cyclic code decoded by its
// block rows (LayeredQcView).
#pragma once

#include <stdint.h>

#include "ldpc_crc.hpp"
#include "ldpc_kernels.hpp"
#include "ldpc_layers.hpp"
#include "ldpc_rate_match.hpp"

namespace ldpc {

struct LayeredView {
  const uint32_t *rows;   // M: first edge | degree << 16
  const uint16_t *ci;     // E: column of CSR edge e
  const uint16_t *order;  // M: rows sorted by layer
  const uint32_t *off;    // L + 1: layer offsets into order
  int M, N, E, KB, L;
};

// A quasi-cyclic code as the circulant route reads it (ldpc_qc.hpp QcTables).
// E may exceed 16 bits: the base tables hold no edge index.
struct LayeredQcView {
  const uint32_t *rows;  // mb: degree (>= 1) | entries before << 16, per block row that has any
  const uint32_t *ent;   // per base entry: block column * Z | shift << 16; 16 zero words behind
  int M, N, E, KB, mb, Z;  // mb: the block rows listed in `rows`
};

enum { kLayeredF64 = 0, kLayeredF32 = 1, kLayeredQ8 = 2 };

// The arithmetic of a decode.  kLayeredF64 / kLayeredF32: `scale` is the
// normalisation factor, 0 < scale <= 1.  kLayeredQ8: `num` is the
// normalisation numerator, 1..16 (the factor is num / 16), and `llr_scale` what
// a sample is multiplied by before it is rounded to an integer in [-127, 127].
struct LayeredArith {
  int kind;
  double scale;
  int num;
  float llr_scale;
};

// Launches one layered decode of args.B frames on `stream` with the layout
// `lay` (layered_layout, or layered_q8_layout for kLayeredQ8: it fits).
// args.ticket / ticket_base / static_stride as in DecodeArgs (`waves` is set
// here: the resident workgroups).  *advance_out: what the launch adds to its
// counter.  *resident: the workgroups the device holds of the kernel this
// arithmetic and layout select (0: not looked up yet).  Returns 0, or -3 on a
// launch error.  rm: the frames are rate-matched samples (ldpc_rate_match.hpp)
// and the frame load recovers them -- args.cw_stride is the frames' stride,
// args.elem_stride 1; a kernel of its own, so `resident` is that kernel's.
// crc: the block's remainder (ldpc_crc.hpp) is evaluated wherever the syndrome
// is and stored at crc->out[frame]; again kernels of their own.
int launch_layered_decode(const LayeredView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          const LayeredArith &ar, void *stream, int *resident,
                          uint32_t *advance_out, const RmArgs *rm = nullptr,
                          const CrcArgs *crc = nullptr);

// The same for a quasi-cyclic code decoded by its block rows: `lay` is the
// layout for mb layers of Z rows with nothing staged (lay.total == lay.frame:
// the base tables are read through the scalar cache).
int launch_layered_decode(const LayeredQcView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          const LayeredArith &ar, void *stream, int *resident,
                          uint32_t *advance_out, const RmArgs *rm = nullptr,
                          const CrcArgs *crc = nullptr);

}  // namespace ldpc
