// ldpc_layered.hip -- layered (row-serial) normalized min-sum for gfx950
// (MI355X): one frame per persistent workgroup, the frame's posteriors LQ[N]
// and check messages R[E] in LDS from the first iteration to the last.
//
// The reference has only the flooding schedule and plain min-sum
// (lib/ldpc_decoder_cb_impl.cc:309-412); this decoder keeps its conventions
// (Lci = -tx, sign(0) = 0, the DBL_MAX seed of the minimum, decision LQ < 0,
// min-sum's exit rule :406-408) and changes the schedule: the rows of H are
// taken layer by layer (ldpc_layers.hpp), each row reading the posteriors the
// rows before it have already updated, and every check message is multiplied
// by a normalisation factor.  Per row j with edges e_0..e_{d-1} in ascending
// column c_0 < ... < c_{d-1}:
//
//   q_k  = LQ[c_k] - R[e_k]
//   s_k  = sign(q_k), P = s_0 * ... * s_{d-1}
//   lo_k = min(BIG, |q_t| for t != k)          (strict <: NaN and inf never win)
//   R[e_k]  = a * ((Real)(P * s_k) * lo_k)     (only the multiply by a rounds)
//   LQ[c_k] = q_k + R[e_k]
//
// A thread owns a row of the current layer.  The rows of a layer share no
// column, so a thread's LQ and R cells are its own until the barrier that ends
// the layer.  The leave-one-out minimum is the smaller of the row's two
// smallest |q| (the second where k is the place of the first): the same value,
// hence the same bits, as the scan over t != k.  No arithmetic here contracts
// (-ffp-contract=off) and none is transcendental, so the f64 precisions are
// one kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ldpc_layered.hpp"
#include "ldpc_layered_dev.hpp"

namespace ldpc {
namespace {

struct LyTabs {
  const uint32_t *rows;
  const uint16_t *ci;
  const uint16_t *order;
  const uint32_t *off;
};

template <typename T>
__device__ __forceinline__ void ly_copy(T *dst, const T *src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// Rows of at most kRowRegs edges are gathered whole into registers: the
// row's column indices in one batch of independent LDS reads, its operands in
// a second, where a loop over the places would wait for each read in turn
// (such chains are what the on-chip kernels' time is).
constexpr int kRowRegs = 8;

// Syndrome weight of the decisions LQ < 0 (checkFrame :236-253, no
// threshold), read from the posteriors in LDS: every thread gets the sum
// (ly_sum_waves: one barrier).
template <typename Real>
__device__ __forceinline__ int ly_syndrome(const LyTabs &g, int M, const Real *LQ, int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  int cnt = 0;
  for (int j0 = 0; j0 < M; j0 += T) {  // uniform trip count: the ballots see whole waves
    const int j = j0 + tid;
    bool odd = false;
    if (j < M) {
      const uint32_t rec = g.rows[j];
      const int e0 = rec & 0xffff, d = rec >> 16;
      if (d > 0 && d <= kRowRegs) {
        int c[kRowRegs];
#pragma unroll
        for (int k = 0; k < kRowRegs; ++k) c[k] = g.ci[e0 + (k < d ? k : 0)];
#pragma unroll
        for (int k = 0; k < kRowRegs; ++k) odd ^= (LQ[c[k]] < Real(0)) & (k < d);
      } else {
        for (int t = 0; t < d; ++t) odd ^= LQ[g.ci[e0 + t]] < Real(0);
      }
    }
    cnt += __popcll(__ballot(odd));
  }
  return ly_sum_waves(cnt, red);
}

template <typename Real, bool STAGED>
__global__ void __launch_bounds__(kLayeredMaxThreads)
    layered_decode_kernel(LayeredView gv, DecodeArgs a, LayeredLayout lay, Real scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  Real *LQ = reinterpret_cast<Real *>(smem);
  Real *R = reinterpret_cast<Real *>(smem + lay.r);
  uint8_t *hard = smem + lay.hard;
  int *red = reinterpret_cast<int *>(smem + lay.red);
  const int tid = threadIdx.x, T = blockDim.x;
  const int M = gv.M, N = gv.N, E = gv.E, NL = gv.L;
  LyTabs g;
  if constexpr (STAGED) {
    uint32_t *rows = reinterpret_cast<uint32_t *>(smem + lay.rows);
    uint16_t *ci = reinterpret_cast<uint16_t *>(smem + lay.ci);
    uint16_t *order = reinterpret_cast<uint16_t *>(smem + lay.order);
    uint32_t *off = reinterpret_cast<uint32_t *>(smem + lay.off);
    ly_copy(rows, gv.rows, M);
    ly_copy(ci, gv.ci, E);
    ly_copy(order, gv.order, M);
    ly_copy(off, gv.off, NL + 1);
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
    ly_load_frame(a, b, N, E, LQ, R);
    int used = 0, weight = 0;
    for (int h = 0;; ++h) {
      for (int l = 0; l < NL; ++l) {
        const int r1 = (int)g.off[l + 1];
        for (int r = (int)g.off[l] + tid; r < r1; r += T) {
          const uint32_t rec = g.rows[g.order[r]];
          const int e0 = rec & 0xffff, d = rec >> 16;
          // the sign product, the two smallest |q| and the place of the smallest
          int P = 1, at = -1;
          Real m1 = Lim<Real>::big(), m2 = Lim<Real>::big();
          if (d > 0 && d <= kRowRegs) {
            // the whole row in registers; places past d read place 0 again and
            // hold +inf, which leaves P, m1, m2 and `at` as they are (sign +1,
            // never below a minimum), so the scan has no branches
            int c[kRowRegs];
            Real q[kRowRegs];
#pragma unroll
            for (int k = 0; k < kRowRegs; ++k) c[k] = g.ci[e0 + (k < d ? k : 0)];
#pragma unroll
            for (int k = 0; k < kRowRegs; ++k) {
              const Real v = LQ[c[k]] - R[e0 + (k < d ? k : 0)];
              q[k] = k < d ? v : (Real)INFINITY;
            }
#pragma unroll
            for (int k = 0; k < kRowRegs; ++k) {
              P *= ly_sgn(q[k]);
              const Real v = Lim<Real>::abs_(q[k]);
              const bool first = v < m1, second = v < m2;
              m2 = first ? m1 : second ? v : m2;
              m1 = first ? v : m1;
              at = first ? k : at;
            }
#pragma unroll
            for (int k = 0; k < kRowRegs; ++k) {
              if (k < d) {
                const Real lo = k == at ? m2 : m1;
                const Real m = scale * ((Real)(P * ly_sgn(q[k])) * lo);
                R[e0 + k] = m;
                LQ[c[k]] = q[k] + m;
              }
            }
            continue;
          }
          for (int k = 0; k < d; ++k) {
            const Real q = LQ[g.ci[e0 + k]] - R[e0 + k];
            P *= ly_sgn(q);
            const Real v = Lim<Real>::abs_(q);
            if (v < m1) {
              m2 = m1;
              m1 = v;
              at = k;
            } else if (v < m2) {
              m2 = v;
            }
          }
          // q_k again (the same operands, the same bits), then the row's writes
          for (int k = 0; k < d; ++k) {
            const int c = g.ci[e0 + k];
            const Real q = LQ[c] - R[e0 + k];
            const Real lo = k == at ? m2 : m1;
            const Real m = scale * ((Real)(P * ly_sgn(q)) * lo);
            R[e0 + k] = m;
            LQ[c] = q + m;
          }
        }
        __syncthreads();
      }
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period (:406-408)
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        weight = ly_syndrome(g, M, LQ, red);
        if (last || weight == 0) break;
      }
    }
    ly_store_frame(a, b, M, N, gv.KB, used, weight, LQ, hard);
    b = ly_next_frame(a, b, red);
  }
}

template <typename Real, bool STAGED>
int launch_kernel(const LayeredView &g, DecodeArgs a, const LayeredLayout &lay, double scale,
                  hipStream_t st, int &resident) {
  const void *fn = (const void *)layered_decode_kernel<Real, STAGED>;
  if (!ly_resident(fn, lay.threads, lay.total, resident)) return -3;
  a.waves = (int)std::min<int64_t>(a.B, resident);
  hipLaunchKernelGGL((layered_decode_kernel<Real, STAGED>), dim3((unsigned)a.waves),
                     dim3((unsigned)lay.threads), (size_t)lay.total, st, g, a, lay, (Real)scale);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int launch_layered_decode(const LayeredView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          double scale, int prec, void *stream, int *resident,
                          uint32_t *advance_out) {
  *advance_out = 0;
  if (args.B <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (prec == 1)
    rc = lay.staged ? launch_kernel<float, true>(g, args, lay, scale, st, resident[1])
                    : launch_kernel<float, false>(g, args, lay, scale, st, resident[1]);
  else
    rc = lay.staged ? launch_kernel<double, true>(g, args, lay, scale, st, resident[0])
                    : launch_kernel<double, false>(g, args, lay, scale, st, resident[0]);
  // one add per frame decoded, each workgroup's last being the one past the batch
  if (rc == 0 && !args.static_stride) *advance_out = (uint32_t)args.B;
  return rc;
}

}  // namespace ldpc
