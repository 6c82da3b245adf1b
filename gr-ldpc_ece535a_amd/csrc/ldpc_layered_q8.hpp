// ldpc_layered_q8.hpp -- host/device interface of the fixed-point layered
// min-sum decoder (ldpc_layered_q8.hip): the float decoder's schedule, plan,
// tables and frame queue (ldpc_layered.hpp) with int8 check messages and int16
// posteriors in LDS.
#pragma once

#include <stdint.h>

#include "ldpc_layered.hpp"

namespace ldpc {

// Launches one fixed-point layered decode of args.B frames on `stream` with
// the layout `lay` (layered_q8_layout: it fits).  num: the normalisation
// numerator, 1..16 (the factor is num / 16); llr_scale: what a sample is
// multiplied by before it is rounded to an integer in [-127, 127].  The views,
// args, *advance_out and the return value are launch_layered_decode's;
// *resident: the workgroups the device holds of the kernel this layout selects
// (0: not looked up yet).
int launch_layered_q8_decode(const LayeredView &g, const DecodeArgs &args,
                             const LayeredLayout &lay, int num, float llr_scale, void *stream,
                             int *resident, uint32_t *advance_out);

// The same for a quasi-cyclic code decoded by its block rows; g.E may exceed 16
// bits (the base tables hold no edge index).
int launch_layered_q8_qc_decode(const LayeredQcView &g, const DecodeArgs &args,
                                const LayeredLayout &lay, int num, float llr_scale, void *stream,
                                int *resident, uint32_t *advance_out);

}  // namespace ldpc
