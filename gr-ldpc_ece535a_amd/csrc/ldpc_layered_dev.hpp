// ldpc_layered_dev.hpp -- what the two layered kernels (ldpc_layered.hip: any
// CSR H through per-edge tables; ldpc_layered_qc.hip: quasi-cyclic codes from
// their base matrix) share on the device: the limits of a precision, the
// per-frame prologue and epilogue, the frame queue, and the host's look-up of
// the workgroups a device holds.  What differs between them is a layer.
#pragma once

#include <hip/hip_runtime.h>

#include <float.h>

#include "ldpc_kernels.hpp"
#include "ldpc_layers.hpp"

namespace ldpc {
namespace {

template <typename Real>
struct Lim;
template <>
struct Lim<double> {
  static __device__ __forceinline__ double big() { return DBL_MAX; }
  static __device__ __forceinline__ double abs_(double x) { return ::fabs(x); }
};
template <>
struct Lim<float> {
  static __device__ __forceinline__ float big() { return FLT_MAX; }
  static __device__ __forceinline__ float abs_(float x) { return ::fabsf(x); }
};

template <typename Real>
__device__ __forceinline__ int ly_sgn(Real v) {
  return (v > Real(0)) - (v < Real(0));
}

// Frame b into LDS: LQ = Lci = -tx, tx = in * polarity (:149-153, :318-321),
// R = 0; ends with the barrier that lets the first layer read them.  The
// layered entry points take strided frames only (no window lists, no
// second-polarity half: DecodeArgs::win and pm_half are unset).
template <typename Real>
__device__ __forceinline__ void ly_load_frame(const DecodeArgs &a, int64_t b, int N, int E,
                                              Real *LQ, Real *R) {
  const int tid = threadIdx.x, T = blockDim.x;
  const float pol = a.polarity;
  const float *src = a.in + b * a.cw_stride;
  for (int i = tid; i < N; i += T) {
    float tx = src[(int64_t)i * a.elem_stride] * pol;
    // two operations: folded into one multiply by -polarity, a NaN sample
    // would keep the sign that negating tx flips
    asm volatile("" : "+v"(tx));
    LQ[i] = (Real)(-tx);
  }
  for (int e = tid; e < E; e += T) R[e] = Real(0);
  __syncthreads();
}

// The per-wave syndrome counts summed over the workgroup: every thread gets
// the sum.  One barrier; the layers' barriers separate this call's reads of
// red[] from the next call's writes.
__device__ __forceinline__ int ly_sum_waves(int cnt, int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  int w = 0;
  const int nwaves = T >> 6;
  for (int i = 0; i < nwaves; ++i) w += red[i];
  return w;
}

// Frame b's outputs (the syndrome's barrier is behind every LQ write): the
// decisions LQ < 0, the iterations used and the syndrome weight, the float
// posteriors, and the info bits M.., MSB first (:207-219).
template <typename Real>
__device__ __forceinline__ void ly_store_frame(const DecodeArgs &a, int64_t b, int M, int N,
                                               int KB, int used, int weight, const Real *LQ,
                                               uint8_t *hard) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int i = tid; i < N; i += T) hard[i] = LQ[i] < Real(0);
  __syncthreads();
  if (tid == 0) {
    if (a.iters) a.iters[b] = used;
    if (a.synd) a.synd[b] = weight;
  }
  if (a.bits)
    for (int i = tid; i < N; i += T) a.bits[b * N + i] = hard[i];
  if (a.llr)
    for (int i = tid; i < N; i += T) a.llr[b * N + i] = (float)LQ[i];
  for (int p = tid; p < KB; p += T) {
    uint32_t o = 0;
    for (int j = 0; j < 8; ++j) {
      const int c = M + 8 * p + j;
      if (c < N) o |= (uint32_t)hard[c] << (7 - j);
    }
    a.packed[b * KB + p] = (uint8_t)o;
  }
}

// The workgroup's next frame (the barrier also ends this frame's LDS reads):
// a fixed stride, or the stream's counter.
__device__ __forceinline__ int64_t ly_next_frame(const DecodeArgs &a, int64_t b, int *red) {
  if (a.static_stride) {
    __syncthreads();
    return b + a.waves;
  }
  if (threadIdx.x == 0) red[16] = (int)(atomicAdd(a.ticket, 1u) - a.ticket_base);
  __syncthreads();
  return (int64_t)a.waves + (int64_t)red[16];
}

// The workgroups the device holds of kernel `fn` at `threads` threads and
// `bytes` of dynamic LDS (looked up once per kernel and layout: resident ==
// 0).  The LDS attribute belongs to the kernel, not to the caller: it allows
// any layout layered_layout accepts.  False on a runtime error.
inline bool ly_resident(const void *fn, int threads, int bytes, int &resident) {
  if (resident != 0) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLayeredLdsLimit) !=
      hipSuccess)
    return false;
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, (size_t)bytes) !=
          hipSuccess ||
      per_cu < 1 || hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    return false;
  resident = per_cu * cus;
  return true;
}

}  // namespace
}  // namespace ldpc
