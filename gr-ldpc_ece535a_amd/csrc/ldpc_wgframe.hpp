// ldpc_wgframe.hpp -- what the workgroup-per-frame kernels share around their
// arithmetic: the on-chip flooding kernels (ldpc_onchip.hip) and the layered
// kernels (ldpc_layered.hip) each decode one frame at a time in a persistent
// workgroup's LDS.  A frame's samples and their sign, the workgroup's
// reduction words, a frame's outputs and the frame queue are stated here once.
// Device code only; the limits and the `red` layout are in ldpc_wglimits.hpp.
//
// The frame queue is DecodeArgs::ticket (ldpc_kernels.hpp).  Its device half is
// wg_next_frame below; its host half is bind_queue / commit_queue
// (ldpc_capi_queues.hip), which hand a launch the counter and its base and
// advance the base by what wg_launch (ldpc_dispatch.hpp) says the launch adds:
// B, one add per frame decoded, each workgroup's last being the one past the
// batch.  A frame index is below B only if the two agree.
#pragma once

#include <hip/hip_runtime.h>

#include "ldpc_kernels.hpp"
#include "ldpc_wglimits.hpp"

namespace ldpc {

// tx = in * polarity, then Lci = -tx (lib/ldpc_decoder_cb_impl.cc:149-153,
// :318-321) as an operation of its own, as in the reference: folded into one
// multiply by -polarity, a NaN sample would keep the sign that negating tx
// flips, and the posteriors it reaches would differ in their sign bit.
__device__ __forceinline__ float lci_of(float in, float polarity) {
  float tx = in * polarity;
  asm volatile("" : "+v"(tx));
  return -tx;
}

// The same as a term of a sum (rate matching's combine, ldpc_rate_match.hpp):
// the negated value in a register of its own, so that the add takes -tx and
// not a subtraction of tx -- the same value, but a NaN's sign would differ.
__device__ __forceinline__ float lci_term_of(float in, float polarity) {
  float v = lci_of(in, polarity);
  asm volatile("" : "+v"(v));
  return v;
}

// Frame b's first sample and polarity: a window of a list (DecodeArgs::win),
// or strided frames whose second half, in a both-polarities launch
// (DecodeArgs::pm_half), re-reads the first half's frames negated.
__device__ __forceinline__ const float *frame_src(const DecodeArgs &a, int64_t b, float &pol) {
  if (a.win) {
    const int64_t w = a.win[b];
    pol = (w & 1) ? -a.polarity : a.polarity;
    return a.in + (w >> 1) * a.elem_stride;
  }
  pol = a.polarity;
  if (a.pm_half > 0 && b >= a.pm_half) {
    b -= a.pm_half;
    pol = -pol;
  }
  return a.in + b * a.cw_stride;
}

// A table into LDS, the workgroup's threads striding over it.
template <typename T>
__device__ __forceinline__ void wg_copy(T *dst, const T *src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// Per-wave counts summed over the workgroup through red[0, kWgRedWaves): every
// thread gets the sum.  One barrier; the caller's next barrier separates this
// call's reads of red[] from the next call's writes.
__device__ __forceinline__ int wg_sum_waves(int cnt, int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  int w = 0;
  const int nwaves = T >> 6;
  for (int i = 0; i < nwaves; ++i) w += red[i];
  return w;
}

// Frame b's outputs: the iterations used and the syndrome weight, the
// decisions bit(i), the float posteriors llr(i), and the info bits M..,
// packed MSB first (:207-219).  The caller's last barrier is behind every
// write that bit and llr read.  The layered kernels' store; the on-chip
// kernel keeps a copy of this body (ldpc_onchip.hip says why).
template <typename Bit, typename Llr>
__device__ __forceinline__ void wg_store_frame(const DecodeArgs &a, int64_t b, int M, int N, int KB,
                                               int used, int weight, const Bit &bit,
                                               const Llr &llr) {
  const int tid = threadIdx.x, T = blockDim.x;
  if (tid == 0) {
    if (a.iters) a.iters[b] = used;
    if (a.synd) a.synd[b] = weight;
  }
  if (a.bits)
    for (int i = tid; i < N; i += T) a.bits[b * N + i] = bit(i);
  if (a.llr)
    for (int i = tid; i < N; i += T) a.llr[b * N + i] = llr(i);
  for (int p = tid; p < KB; p += T) {
    uint32_t o = 0;
    for (int j = 0; j < 8; ++j) {
      const int c = M + 8 * p + j;
      if (c < N) o |= bit(c) << (7 - j);
    }
    a.packed[b * KB + p] = (uint8_t)o;
  }
}

// The workgroup's next frame after frame b (the barrier also ends this
// frame's LDS reads): a fixed stride of a.waves workgroups
// (DecodeArgs::static_stride), or one add on the stream's counter by thread 0,
// handed to the workgroup through red[kWgRedNext].
__device__ __forceinline__ int64_t wg_next_frame(const DecodeArgs &a, int64_t b, int *red) {
  if (a.static_stride) {
    __syncthreads();
    return b + a.waves;
  }
  if (threadIdx.x == 0) red[kWgRedNext] = (int)(atomicAdd(a.ticket, 1u) - a.ticket_base);
  __syncthreads();
  return (int64_t)a.waves + (int64_t)red[kWgRedNext];
}

}  // namespace ldpc
