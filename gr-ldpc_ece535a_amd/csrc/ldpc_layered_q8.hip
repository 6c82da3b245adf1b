// ldpc_layered_q8.hip -- fixed-point layered normalized min-sum for gfx950
// (MI355X): the schedule, plan, exit rule, outputs and frame queue of
// ldpc_layered.hip / ldpc_layered_qc.hip (one frame per persistent workgroup,
// its state in LDS from the first iteration to the last), with the check
// messages R[E] as int8 and the posteriors LQ[N] as int16: a frame is
// a16(2 N) + a16(E) + 128 bytes where the float kernels need 5 N + 4 E.  (The
// reference has neither a layered schedule nor fixed point:
// lib/ldpc_decoder_cb_impl.cc:309-412 is flooding min-sum in double.)
//
// The contract (include/ldpc_hip.h), num in [1, 16]:
//
//   tx_i = in_i * polarity;  v_i = (-tx_i) * llr_scale          (float)
//   LQ[i] = v_i is NaN ? 0 : clamp(rint(v_i), -127, 127);  R[e] = 0
//   per iteration, layer, row of it, edges e_k in ascending column c_k:
//     q_k  = LQ[c_k] - R[e_k]
//     s_k  = q_k < 0 ? -1 : +1,  P = s_0 * ... * s_{d-1}
//     lo_k = min(127, |q_t| for t != k)
//     R[e_k]  = (P * s_k) * ((lo_k * num + 8) >> 4)
//     LQ[c_k] = q_k + R[e_k]
//
// All of it is integer arithmetic in 32-bit registers; what is stored fits its
// type exactly: |R| <= 127, and LQ[c] = Lc_c + the sum of the column's R after
// every update, so |LQ| <= 127 (dv + 1) <= 32767 (layered_q8_layout checks dv).
// The sign product is the XOR of the q's sign bits; the leave-one-out minimum is
// the smaller of the row's two smallest |q| under the seed 127 (the second at
// the place of the first), as in the float kernels.  The decisions are LQ < 0,
// read in place: there is no decision array.
//
// Two routes, which differ in how a row finds its columns and messages and
// share everything else: per-edge tables for any plan (ldpc_layered.hip's
// LayeredView, a thread per row of the layer) and the base matrix of a
// quasi-cyclic code decoded by its block rows (ldpc_layered_qc.hip's
// LayeredQcView, thread i < Z on row r * Z + i, R place-major within the block
// row).  Consecutive lanes touch consecutive bytes of R and, up to the wrap,
// consecutive halfwords of LQ: four and two lanes to a dword.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ldpc_layered_dev.hpp"
#include "ldpc_layered_q8.hpp"
#include "ldpc_qc.hpp"

namespace ldpc {
namespace {

constexpr int kQ8Max = 127;
// what a place past the row's degree holds: sign +, never below a minimum
constexpr int kQ8Pad = 32767;
constexpr int kRegsShort = 8, kRegsLong = 16;
static_assert(kRegsLong <= kQcEntPad, "a register row is loaded whole from any entry");

// ---- the row update, shared by both routes -------------------------------------

// The XOR of the q's (its sign bit is that of P), the two smallest |q| below
// the seed and the place of the smallest.
struct Q8Row {
  int sg = 0, m1 = kQ8Max, m2 = kQ8Max, at = -1;
};

__device__ __forceinline__ void q8_scan(Q8Row &s, int q, int k) {
  s.sg ^= q;
  const int v = q < 0 ? -q : q;
  const bool first = v < s.m1, second = v < s.m2;
  s.m2 = first ? s.m1 : second ? v : s.m2;
  s.m1 = first ? v : s.m1;
  s.at = first ? k : s.at;
}

__device__ __forceinline__ int q8_msg(const Q8Row &s, int q, int k, int num) {
  const int lo = k == s.at ? s.m2 : s.m1;
  const int mag = (lo * num + 8) >> 4;
  return (s.sg ^ q) < 0 ? -mag : mag;
}

// A row of d <= D places whole in registers: the columns in one batch of
// reads, both operands of every place in a second.  Places past d read some
// column of the code (col_pad) and the message of place 0, and hold kQ8Pad, so
// the scan has no branches.  A: where place k's column (col) and message (msg)
// are.
template <int D, typename A>
__device__ __forceinline__ void q8_row_regs(const A &ad, int d, int16_t *LQ, int8_t *R, int num) {
  int c[D], e[D], q[D], rv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    c[k] = ad.col_pad(k, d);
    e[k] = ad.msg(k < d ? k : 0);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = LQ[c[k]];
#pragma unroll
  for (int k = 0; k < D; ++k) rv[k] = R[e[k]];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = k < d ? q[k] - rv[k] : kQ8Pad;
  Q8Row s;
#pragma unroll
  for (int k = 0; k < D; ++k) q8_scan(s, q[k], k);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (k < d) {
      const int m = q8_msg(s, q[k], k, num);
      R[e[k]] = (int8_t)m;
      LQ[c[k]] = (int16_t)(q[k] + m);
    }
  }
}

// A longer row: the scan, then q_k again (the same operands) and the row's writes.
template <typename A>
__device__ __forceinline__ void q8_row_loop(const A &ad, int d, int16_t *LQ, int8_t *R, int num) {
  Q8Row s;
#pragma unroll 4
  for (int k = 0; k < d; ++k) q8_scan(s, (int)LQ[ad.col(k)] - (int)R[ad.msg(k)], k);
#pragma unroll 4
  for (int k = 0; k < d; ++k) {
    const int c = ad.col(k), e = ad.msg(k);
    const int q = (int)LQ[c] - (int)R[e];
    const int m = q8_msg(s, q, k, num);
    R[e] = (int8_t)m;
    LQ[c] = (int16_t)(q + m);
  }
}

// ---- prologue and epilogue, shared by both routes --------------------------------

// Frame b into LDS: LQ = the quantised -tx * llr_scale, R = 0 (as dwords: R's
// region is a multiple of 16 bytes); ends with the barrier that lets the first
// layer read them.  Strided frames only, as ly_load_frame.
__device__ __forceinline__ void q8_load_frame(const DecodeArgs &a, int64_t b, int N, int r_dwords,
                                              float llr_scale, int16_t *LQ, uint32_t *R32) {
  const int tid = threadIdx.x, T = blockDim.x;
  const float pol = a.polarity;
  const float *src = a.in + b * a.cw_stride;
  for (int i = tid; i < N; i += T) {
    float tx = src[(int64_t)i * a.elem_stride] * pol;
    // negated as an operation of its own (ly_load_frame)
    asm volatile("" : "+v"(tx));
    const float v = (-tx) * llr_scale;
    const float c = fminf(fmaxf(rintf(v), -(float)kQ8Max), (float)kQ8Max);
    LQ[i] = v != v ? (int16_t)0 : (int16_t)(int)c;
  }
  for (int e = tid; e < r_dwords; e += T) R32[e] = 0u;
  __syncthreads();
}

// Frame b's outputs (the syndrome's barrier is behind every LQ write).
__device__ __forceinline__ void q8_store_frame(const DecodeArgs &a, int64_t b, int M, int N, int KB,
                                               int used, int weight, const int16_t *LQ) {
  const int tid = threadIdx.x, T = blockDim.x;
  if (tid == 0) {
    if (a.iters) a.iters[b] = used;
    if (a.synd) a.synd[b] = weight;
  }
  if (a.bits)
    for (int i = tid; i < N; i += T) a.bits[b * N + i] = LQ[i] < 0;
  if (a.llr)
    for (int i = tid; i < N; i += T) a.llr[b * N + i] = (float)LQ[i];
  for (int p = tid; p < KB; p += T) {
    uint32_t o = 0;
    for (int j = 0; j < 8; ++j) {
      const int c = M + 8 * p + j;
      if (c < N) o |= (uint32_t)(LQ[c] < 0) << (7 - j);
    }
    a.packed[b * KB + p] = (uint8_t)o;
  }
}

// ---- the table route -----------------------------------------------------------

struct Q8Tabs {
  const uint32_t *rows;
  const uint16_t *ci;
  const uint16_t *order;
  const uint32_t *off;
};

struct TabAddr {
  const uint16_t *ci;
  int e0;
  __device__ __forceinline__ int col(int k) const { return ci[e0 + k]; }
  __device__ __forceinline__ int col_pad(int k, int d) const { return ci[e0 + (k < d ? k : 0)]; }
  __device__ __forceinline__ int msg(int k) const { return e0 + k; }
};

template <typename T>
__device__ __forceinline__ void q8_copy(T *dst, const T *src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// Syndrome weight of the decisions LQ < 0, every thread gets the sum
// (ly_sum_waves: one barrier).
__device__ __forceinline__ int q8_syndrome(const Q8Tabs &g, int M, const int16_t *LQ, int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  int cnt = 0;
  for (int j0 = 0; j0 < M; j0 += T) {  // uniform trip count: the ballots see whole waves
    const int j = j0 + tid;
    int x = 0;
    if (j < M) {
      const uint32_t rec = g.rows[j];
      const int e0 = rec & 0xffff, d = rec >> 16;
      if (d > 0 && d <= kRegsShort) {
        int c[kRegsShort];
#pragma unroll
        for (int k = 0; k < kRegsShort; ++k) c[k] = g.ci[e0 + (k < d ? k : 0)];
#pragma unroll
        for (int k = 0; k < kRegsShort; ++k) x ^= k < d ? (int)LQ[c[k]] : 0;
      } else {
        for (int t = 0; t < d; ++t) x ^= (int)LQ[g.ci[e0 + t]];
      }
    }
    cnt += __popcll(__ballot(x < 0));
  }
  return ly_sum_waves(cnt, red);
}

template <bool STAGED>
__global__ void __launch_bounds__(kLayeredMaxThreads)
    layered_q8_kernel(LayeredView gv, DecodeArgs a, LayeredLayout lay, int num, float llr_scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  int16_t *LQ = reinterpret_cast<int16_t *>(smem);
  int8_t *R = reinterpret_cast<int8_t *>(smem + lay.r);
  int *red = reinterpret_cast<int *>(smem + lay.red);
  const int tid = threadIdx.x, T = blockDim.x;
  const int M = gv.M, N = gv.N, NL = gv.L;
  const int r_dwords = (lay.red - lay.r) >> 2;
  Q8Tabs g;
  if constexpr (STAGED) {
    uint32_t *rows = reinterpret_cast<uint32_t *>(smem + lay.rows);
    uint16_t *ci = reinterpret_cast<uint16_t *>(smem + lay.ci);
    uint16_t *order = reinterpret_cast<uint16_t *>(smem + lay.order);
    uint32_t *off = reinterpret_cast<uint32_t *>(smem + lay.off);
    q8_copy(rows, gv.rows, M);
    q8_copy(ci, gv.ci, gv.E);
    q8_copy(order, gv.order, M);
    q8_copy(off, gv.off, NL + 1);
    g.rows = rows;
    g.ci = ci;
    g.order = order;
    g.off = off;
    __syncthreads();
  } else {
    g.rows = gv.rows;
    g.ci = gv.ci;
    g.order = gv.order;
    g.off = gv.off;
  }

  int64_t b = blockIdx.x;
  while (b < a.B) {
    q8_load_frame(a, b, N, r_dwords, llr_scale, LQ, reinterpret_cast<uint32_t *>(R));
    int used = 0, weight = 0;
    for (int h = 0;; ++h) {
      for (int l = 0; l < NL; ++l) {
        const int r1 = (int)g.off[l + 1];
        for (int r = (int)g.off[l] + tid; r < r1; r += T) {
          const uint32_t rec = g.rows[g.order[r]];
          const int d = rec >> 16;
          const TabAddr ad{g.ci, (int)(rec & 0xffff)};
          if (d > 0 && d <= kRegsShort)
            q8_row_regs<kRegsShort>(ad, d, LQ, R, num);
          else
            q8_row_loop(ad, d, LQ, R, num);
        }
        __syncthreads();
      }
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        weight = q8_syndrome(g, M, LQ, red);
        if (last || weight == 0) break;
      }
    }
    q8_store_frame(a, b, M, N, gv.KB, used, weight, LQ);
    b = ly_next_frame(a, b, red);
  }
}

// ---- the circulant route -------------------------------------------------------

// The base tables through the constant address space: a uniform index is a
// scalar load whatever the kernel stores in between (ldpc_layered_qc.hip).
typedef const uint32_t __attribute__((address_space(4))) *QcWords;
__device__ __forceinline__ QcWords qc_words(const uint32_t *p) {
  return (QcWords)(uintptr_t)p;
}

// Column of lane i's edge in the circulant w = c * Z | s << 16.
__device__ __forceinline__ int qc_col(uint32_t w, int i, int Z) {
  const uint32_t t = (uint32_t)i + (w >> 16);
  return (int)((w & 0xffffu) + min(t, t - (uint32_t)Z));
}

// Lane i's row of a block row: place k's column from the entry word, its
// message at r0 + k * Z (r0 = eb * Z + i: R is place-major within the block row).
template <typename W>
struct QcAddr {
  W w;
  int i, Z, r0;
  __device__ __forceinline__ int col(int k) const { return qc_col(w[k], i, Z); }
  // the words past d are other entries of the table or its padding: columns of the code
  __device__ __forceinline__ int col_pad(int k, int) const { return col(k); }
  __device__ __forceinline__ int msg(int k) const { return r0 + k * Z; }
};

// Syndrome weight block row by block row, four side by side
// (ldpc_layered_qc.hip's qc_syndrome): thread i XORs the posteriors at its
// row's places, whose sign is the parity of the decisions.
constexpr int kSynRows = 4;

__device__ __forceinline__ int q8_qc_syndrome(const LayeredQcView &g, const int16_t *LQ, int *red) {
  const int tid = threadIdx.x, Z = g.Z;
  const int i = min(tid, Z - 1);
  const bool mine = tid < Z;
  int cnt = 0;
  for (int r0 = 0; r0 < g.mb; r0 += kSynRows) {  // every wave sees every ballot
    int d[kSynRows];
    QcWords ent[kSynRows];
    uint32_t w[kSynRows][kRegsShort];
#pragma unroll
    for (int s = 0; s < kSynRows; ++s) {
      const bool ok = r0 + s < g.mb;
      const uint32_t rec = qc_words(g.rows)[ok ? r0 + s : 0];
      d[s] = ok ? (int)(rec & 0xffffu) : 0;
      ent[s] = qc_words(g.ent) + (rec >> 16);
    }
#pragma unroll
    for (int s = 0; s < kSynRows; ++s)
#pragma unroll
      for (int k = 0; k < kRegsShort; ++k) w[s][k] = ent[s][k];
    int x[kSynRows];
#pragma unroll
    for (int s = 0; s < kSynRows; ++s) {
      x[s] = 0;
#pragma unroll
      for (int k = 0; k < kRegsShort; ++k) {
        const int v = LQ[qc_col(w[s][k], i, Z)];
        x[s] ^= k < d[s] ? v : 0;
      }
    }
#pragma unroll
    for (int s = 0; s < kSynRows; ++s)
      for (int k = kRegsShort; k < d[s]; ++k) x[s] ^= (int)LQ[qc_col(ent[s][k], i, Z)];
#pragma unroll
    for (int s = 0; s < kSynRows; ++s) cnt += __popcll(__ballot((x[s] < 0) & mine));
  }
  return ly_sum_waves(cnt, red);
}

__global__ void __launch_bounds__(kLayeredMaxThreads)
    layered_q8_qc_kernel(LayeredQcView gv, DecodeArgs a, LayeredLayout lay, int num,
                         float llr_scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  int16_t *LQ = reinterpret_cast<int16_t *>(smem);
  int8_t *R = reinterpret_cast<int8_t *>(smem + lay.r);
  int *red = reinterpret_cast<int *>(smem + lay.red);
  const int tid = threadIdx.x;
  const int M = gv.M, N = gv.N, Z = gv.Z, mb = gv.mb;
  const int r_dwords = (lay.red - lay.r) >> 2;

  int64_t b = blockIdx.x;
  while (b < a.B) {
    q8_load_frame(a, b, N, r_dwords, llr_scale, LQ, reinterpret_cast<uint32_t *>(R));
    int used = 0, weight = 0;
    for (int h = 0;; ++h) {
      int eb = 0;  // the base entries before block row r
      for (int r = 0; r < mb; ++r) {
        QcWords ent = qc_words(gv.ent) + eb;
        const int d = (int)(qc_words(gv.rows)[r] & 0xffffu);
        __builtin_assume(d >= 1);  // the table lists no empty block row
        uint32_t w[kRegsLong];
#pragma unroll
        for (int k = 0; k < kRegsShort; ++k) w[k] = ent[k];
        if (tid < Z) {
          const int r0 = eb * Z + tid;
          if (d <= kRegsShort) {
            q8_row_regs<kRegsShort>(QcAddr<const uint32_t *>{w, tid, Z, r0}, d, LQ, R, num);
          } else if (d <= kRegsLong) {
#pragma unroll
            for (int k = kRegsShort; k < kRegsLong; ++k) w[k] = ent[k];
            q8_row_regs<kRegsLong>(QcAddr<const uint32_t *>{w, tid, Z, r0}, d, LQ, R, num);
          } else {
            q8_row_loop(QcAddr<QcWords>{ent, tid, Z, r0}, d, LQ, R, num);
          }
        }
        __syncthreads();
        eb += d;
      }
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        weight = q8_qc_syndrome(gv, LQ, red);
        if (last || weight == 0) break;
      }
    }
    q8_store_frame(a, b, M, N, gv.KB, used, weight, LQ);
    b = ly_next_frame(a, b, red);
  }
}

template <typename Kernel, typename View>
int launch_kernel(Kernel kernel, const View &g, DecodeArgs a, const LayeredLayout &lay, int num,
                  float llr_scale, hipStream_t st, int &resident, uint32_t *advance_out) {
  *advance_out = 0;
  if (a.B <= 0) return 0;
  if (!ly_resident((const void *)kernel, lay.threads, lay.total, resident)) return -3;
  a.waves = (int)std::min<int64_t>(a.B, resident);
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.waves), dim3((unsigned)lay.threads),
                     (size_t)lay.total, st, g, a, lay, num, llr_scale);
  if (hipGetLastError() != hipSuccess) return -3;
  // one add per frame decoded, each workgroup's last being the one past the batch
  if (!a.static_stride) *advance_out = (uint32_t)a.B;
  return 0;
}

}  // namespace

int launch_layered_q8_decode(const LayeredView &g, const DecodeArgs &args,
                             const LayeredLayout &lay, int num, float llr_scale, void *stream,
                             int *resident, uint32_t *advance_out) {
  hipStream_t st = (hipStream_t)stream;
  return lay.staged ? launch_kernel(layered_q8_kernel<true>, g, args, lay, num, llr_scale, st,
                                    *resident, advance_out)
                    : launch_kernel(layered_q8_kernel<false>, g, args, lay, num, llr_scale, st,
                                    *resident, advance_out);
}

int launch_layered_q8_qc_decode(const LayeredQcView &g, const DecodeArgs &args,
                                const LayeredLayout &lay, int num, float llr_scale, void *stream,
                                int *resident, uint32_t *advance_out) {
  return launch_kernel(layered_q8_qc_kernel, g, args, lay, num, llr_scale, (hipStream_t)stream,
                       *resident, advance_out);
}

}  // namespace ldpc
