// ldpc_layered.hpp -- host/device types of the layered normalized min-sum
// decoder (ldpc_layered.hip): one frame per persistent workgroup, the frame's
// posteriors and check messages in LDS, the rows of H taken layer by layer
// (ldpc_layers.hpp).
#pragma once

#include <stdint.h>

#include "ldpc_kernels.hpp"
#include "ldpc_layers.hpp"

namespace ldpc {

struct LayeredView {
  const uint32_t *rows;   // M: first edge | degree << 16
  const uint16_t *ci;     // E: column of CSR edge e
  const uint16_t *order;  // M: rows sorted by layer
  const uint32_t *off;    // L + 1: layer offsets into order
  int M, N, E, KB, L;
};

// Launches one layered decode of args.B frames on `stream` with the layout
// `lay` (layered_layout: it fits).  args.ticket / ticket_base / static_stride
// as in DecodeArgs (`waves` is set here: the resident workgroups).  scale: the
// normalisation factor, 0 < scale <= 1.  *advance_out: what the launch adds to
// its counter.  resident[prec == 1]: the workgroups the device holds of each
// kernel for this layout (0: not looked up yet).  Returns 0, or -3 on a launch
// error.
int launch_layered_decode(const LayeredView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          double scale, int prec, void *stream, int *resident,
                          uint32_t *advance_out);

// A quasi-cyclic code as the circulant kernel reads it (ldpc_qc.hpp QcTables).
struct LayeredQcView {
  const uint32_t *rows;  // mb: degree (>= 1) | entries before << 16, per block row that has any
  const uint32_t *ent;   // per base entry: block column * Z | shift << 16; 16 zero words behind
  int M, N, E, KB, mb, Z;  // mb: the block rows listed in `rows`
};

// The same launch for a quasi-cyclic code decoded by its block rows
// (ldpc_layered_qc.hip): `lay` is layered_layout's for mb layers of Z rows,
// with nothing staged (lay.total == lay.frame: the base tables are read
// through the scalar cache).  Arguments and result as launch_layered_decode.
int launch_layered_qc_decode(const LayeredQcView &g, const DecodeArgs &args,
                             const LayeredLayout &lay, double scale, int prec, void *stream,
                             int *resident, uint32_t *advance_out);

}  // namespace ldpc
