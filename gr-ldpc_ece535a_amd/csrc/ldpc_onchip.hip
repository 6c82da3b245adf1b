// ldpc_onchip.hip -- on-chip decode kernels for gfx950 (MI355X): one frame
// per workgroup, every message of the frame in LDS from the first iteration
// to the last.
//
// The small-code kernels (ldpc_kernels.hip) stop at E <= 512; the large-code
// kernels (ldpc_graph.hip) keep the messages in HBM and pay two or three
// grid-wide launches per iteration.  A code of a few thousand edges fits the
// 160 KiB of LDS a workgroup may declare, so here a persistent workgroup
// decodes one frame at a time entirely on chip and then takes the next frame
// (ldpc_wgframe.hpp: the frame's source, the wave sum and the queue, shared
// with the layered kernels).  Threads stride over the edges (check pass, bit
// messages), the columns (posterior, hard decision) and the rows (syndrome);
// the passes are separated by workgroup barriers and no workgroup ever waits
// on another.
//
// The per-edge arithmetic is the reference's, in its order (min-sum
// lib/ldpc_decoder_cb_impl.cc:350-403, sum-product :503-553), with the same
// Math<PREC> as the other two paths (ldpc_device.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ldpc_device.hpp"
#include "ldpc_dispatch.hpp"
#include "ldpc_onchip.hpp"
#include "ldpc_wgframe.hpp"

namespace ldpc {
namespace {

template <int PREC>
constexpr int tab_bytes() {
  return Math<PREC>::kTabN > 0 ? (int)sizeof(typename Math<PREC>::Tab) * Math<PREC>::kTabN : 0;
}

// The code's tables as the kernel reads them: LDS copies or global memory.
struct OcTabs {
  const uint32_t *erow;
  const uint2 *ecol;
  const uint32_t *rows;
  const uint32_t *cols;
  const uint16_t *ci;
  const uint16_t *ce;
  int M, N, E;
};

// Syndrome weight of the hard decisions in LDS (checkFrame :236-253, no
// threshold): every thread gets the sum (wg_sum_waves: one barrier).
__device__ __forceinline__ int oc_syndrome(const OcTabs &g, const uint8_t *hard, int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  int cnt = 0;
  for (int j0 = 0; j0 < g.M; j0 += T) {  // uniform trip count: the ballots see whole waves
    const int j = j0 + tid;
    bool odd = false;
    if (j < g.M) {
      const uint32_t rec = g.rows[j];
      const int e0 = rec & 0xffff, d = rec >> 16;
      uint32_t par = 0;
      for (int t = 0; t < d; ++t) par ^= hard[g.ci[e0 + t]];
      odd = par != 0;
    }
    cnt += __popcll(__ballot(odd));
  }
  return wg_sum_waves(cnt, red);
}

// Column i's posterior from the check messages in R: the ascending-row sum
// of (E + r) from 0.0 (sum-product :519-532) or Lci + the ascending sum of
// L(r) (min-sum :379-385).
template <int METHOD, typename Real>
__device__ __forceinline__ Real oc_posterior(const OcTabs &g, const Real *R, const float *chan,
                                             int i) {
  const uint32_t rec = g.cols[i];
  const int k0 = rec & 0xffff, d = rec >> 16;
  const Real rc = (Real)chan[i];
  Real acc = Real(0);
  if constexpr (METHOD == 1) {
    for (int k = 0; k < d; ++k) acc = acc + (R[g.ce[k0 + k]] + rc);
    return acc;
  } else {
    for (int k = 0; k < d; ++k) acc = acc + R[g.ce[k0 + k]];
    return rc + acc;
  }
}

template <int PREC, int METHOD, bool STAGED>
__global__ void __launch_bounds__(kOnchipMaxThreads)
    onchip_decode_kernel(OnchipView gv, DecodeArgs a, OnchipLayout L) {
  typedef typename Math<PREC>::Real Real;
  typedef typename Math<PREC>::Tab Tab;
  extern __shared__ __align__(16) unsigned char smem[];
  Real *A = reinterpret_cast<Real *>(smem);
  Real *R = reinterpret_cast<Real *>(smem + L.r);
  Tab *logtab = reinterpret_cast<Tab *>(smem + L.tab);
  float *chan = reinterpret_cast<float *>(smem + L.chan);
  uint8_t *hard = smem + L.hard;
  int *red = reinterpret_cast<int *>(smem + L.red);
  const int tid = threadIdx.x, T = blockDim.x;
  const int M = gv.M, N = gv.N, E = gv.E;
  if constexpr (METHOD == 1) stage_tab<PREC>(logtab);
  OcTabs g;
  g.M = M;
  g.N = N;
  g.E = E;
  if constexpr (STAGED) {
    uint32_t *erow = reinterpret_cast<uint32_t *>(smem + L.erow);
    uint2 *ecol = reinterpret_cast<uint2 *>(smem + L.ecol);
    uint32_t *rows = reinterpret_cast<uint32_t *>(smem + L.rows);
    uint32_t *cols = reinterpret_cast<uint32_t *>(smem + L.cols);
    uint16_t *ci = reinterpret_cast<uint16_t *>(smem + L.ci);
    uint16_t *ce = reinterpret_cast<uint16_t *>(smem + L.ce);
    wg_copy(erow, gv.erow, E);
    wg_copy(ecol, gv.ecol, E);
    wg_copy(rows, gv.rows, M);
    wg_copy(cols, gv.cols, N);
    wg_copy(ci, gv.ci, E);
    wg_copy(ce, gv.ce, E);
    g.erow = erow;
    g.ecol = ecol;
    g.rows = rows;
    g.cols = cols;
    g.ci = ci;
    g.ce = ce;
    __syncthreads();
  } else {
    g.erow = gv.erow;
    g.ecol = gv.ecol;
    g.rows = gv.rows;
    g.cols = gv.cols;
    g.ci = gv.ci;
    g.ce = gv.ce;
  }

  int64_t b = blockIdx.x;
  while (b < a.B) {
    float pol;
    const float *src = frame_src(a, b, pol);
    // channel samples: tx = in * polarity (:149-153), kept as -tx (Lci :318-321, r :486)
    for (int i = tid; i < N; i += T) chan[i] = lci_of(src[(int64_t)i * a.elem_stride], pol);
    __syncthreads();
    // first bit -> check messages (:328-331, :489-496)
    for (int e = tid; e < E; e += T) {
      const Real m = (Real)chan[g.ecol[e].x & 0xffff];
      if constexpr (METHOD == 1)
        A[e] = Math<PREC>::tanh_half(m, logtab);
      else
        A[e] = m;
    }
    __syncthreads();
    int used = 0, weight = 0;
    for (int h = 0;; ++h) {
      // horizontal step: the row's other edges in ascending column
      for (int e = tid; e < E; e += T) {
        const uint32_t rec = g.erow[e];
        const int e0 = rec & 0xffff, d = (rec >> 16) & 0xff, self = rec >> 24;
        if constexpr (METHOD == 1) {
          Real P = Real(1);  // :506-511
          for (int t = 0; t < d; ++t)
            if (t != self) P = P * A[e0 + t];
          R[e] = Math<PREC>::check_msg(P, logtab);  // :513
        } else {
          const int s = sgn(A[e]);  // :350-376
          int prod = s;
          Real lo = Math<PREC>::max_();
          for (int t = 0; t < d; ++t)
            if (t != self) {
              const Real v = A[e0 + t];
              prod *= sgn(v);
              const Real beta = Math<PREC>::abs_(v);
              lo = beta < lo ? beta : lo;
            }
          R[e] = (Real)(prod * s) * lo;
        }
      }
      __syncthreads();
      // posterior and hard decision per column
      for (int i = tid; i < N; i += T) {
        const Real p = oc_posterior<METHOD>(g, R, chan, i);
        hard[i] = METHOD == 1 ? (p <= Real(0)) : (p < Real(0));
      }
      __syncthreads();
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period
      // (:406-408, :535-537); a frame that stops here runs no message pass
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        weight = oc_syndrome(g, hard, red);
        if (last || weight == 0) break;
      }
      // vertical step: the column's other edges in ascending row
      for (int e = tid; e < E; e += T) {
        const uint2 rec = g.ecol[e];
        const int i = rec.x & 0xffff, self = rec.x >> 16;
        const int k0 = rec.y & 0xffff, d = rec.y >> 16;
        const Real rc = (Real)chan[i];
        Real acc = Real(0);
        if constexpr (METHOD == 1) {  // :540-553
          for (int k = 0; k < d; ++k)
            if (k != self) acc = acc + (R[g.ce[k0 + k]] + rc);
          A[e] = Math<PREC>::tanh_half(acc, logtab);  // :509 of the next iteration
        } else {  // :387-392
          for (int k = 0; k < d; ++k) acc = acc + R[g.ce[k0 + k]];
          A[e] = (rc + acc) - R[e];
        }
      }
      __syncthreads();
    }
    // outputs: R and hard are those of the frame's last iteration
    // A copy of wg_store_frame (ldpc_wgframe.hpp) with bit(i) = hard[i] and
    // llr(i) = oc_posterior: through the helper all 12 kernels kept their
    // registers and changed in code length (-800 to +256 bytes), and the
    // sum-product kernel with its tables in L2 measured 1.4 to 1.7 % slower on
    // every N = 2160 leg (profiles/round19/wgframe_ab.txt, series 1; the
    // lengths: wgframe_isa.txt).  Only that kernel failed; the body stays for
    // all 12 all the same: one copy is less code than the helper and the copy
    // side by side under an `if constexpr`.
    if (tid == 0) {
      if (a.iters) a.iters[b] = used;
      if (a.synd) a.synd[b] = weight;
    }
    if (a.bits)
      for (int i = tid; i < N; i += T) a.bits[b * N + i] = hard[i];
    if (a.llr)
      for (int i = tid; i < N; i += T) a.llr[b * N + i] = (float)oc_posterior<METHOD>(g, R, chan, i);
    for (int p = tid; p < gv.KB; p += T) {  // info bits M.., MSB first (:207-219)
      uint32_t o = 0;
      for (int j = 0; j < 8; ++j) {
        const int c = M + 8 * p + j;
        if (c < N) o |= (uint32_t)hard[c] << (7 - j);
      }
      a.packed[b * gv.KB + p] = (uint8_t)o;
    }
    b = wg_next_frame(a, b, red);
  }
}

int tab_bytes_of(int method, int prec) {
  if (method != 1) return 0;
  return prec == 1 ? tab_bytes<1>() : prec == 3 ? tab_bytes<3>() : tab_bytes<0>();
}

template <int PREC, int METHOD, bool STAGED>
int launch_kernel(const OnchipView &g, DecodeArgs a, const OnchipLayout &L, hipStream_t st,
                  int &resident, uint32_t *advance_out) {
  if (!wg_launch((const void *)onchip_decode_kernel<PREC, METHOD, STAGED>, L.threads, L.total,
                 resident, a, advance_out))
    return -3;
  hipLaunchKernelGGL((onchip_decode_kernel<PREC, METHOD, STAGED>), dim3((unsigned)a.waves),
                     dim3((unsigned)L.threads), (size_t)L.total, st, g, a, L);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int PREC, int METHOD>
int launch_one(const OnchipView &g, const DecodeArgs &a, const OnchipLayout &L, hipStream_t st,
               int &resident, uint32_t *advance_out) {
  return L.staged ? launch_kernel<PREC, METHOD, true>(g, a, L, st, resident, advance_out)
                  : launch_kernel<PREC, METHOD, false>(g, a, L, st, resident, advance_out);
}

}  // namespace

bool onchip_plan(int M, int N, int E, int dc_max, int dv_max, int method, int prec,
                 OnchipLayout &L) {
  const int64_t real = prec == 1 ? 4 : 8;
  LdsCarve c;
  c.take((int64_t)E * real);  // A
  L.r = c.take((int64_t)E * real);
  L.tab = c.take(tab_bytes_of(method, prec));
  L.chan = c.take((int64_t)N * 4);
  L.hard = c.take(N);
  L.red = c.take(kWgRedBytes);
  const int64_t frame = c.end;
  const bool fits = frame <= kOnchipLdsLimit && M <= kOnchipIndexMax && N <= kOnchipIndexMax &&
                    E <= kOnchipIndexMax && dc_max <= kGraphDcMax && dv_max <= kGraphDvMax;
  // the tables behind the frame, where there is room for all of them
  L.erow = c.take((int64_t)E * 4);
  L.ecol = c.take((int64_t)E * 8);
  L.rows = c.take((int64_t)M * 4);
  L.cols = c.take((int64_t)N * 4);
  L.ci = c.take((int64_t)E * 2);
  L.ce = c.take((int64_t)E * 2);
  const bool staged = fits && c.end <= kOnchipLdsLimit;
  L.staged = staged ? 1 : 0;
  L.frame = LdsCarve::sat(frame);
  L.total = LdsCarve::sat(staged ? c.end : frame);
  L.threads = (int)std::min<int64_t>(kOnchipMaxThreads,
                                     std::max<int64_t>(64, ((int64_t)E + 63) / 64 * 64));
  return fits;
}

void onchip_build(int M, int N, const std::vector<int32_t> &rp, const std::vector<int32_t> &ci,
                  const std::vector<int32_t> &cp, const std::vector<int32_t> &ce, OnchipTables &t) {
  const int E = rp[M];
  t.erow.assign((size_t)E, 0);
  t.ecol.assign((size_t)2 * E, 0);
  t.rows.assign((size_t)M, 0);
  t.cols.assign((size_t)N, 0);
  t.ci.assign((size_t)E, 0);
  t.ce.assign((size_t)E, 0);
  for (int j = 0; j < M; ++j) {
    const uint32_t e0 = (uint32_t)rp[j], d = (uint32_t)(rp[j + 1] - rp[j]);
    t.rows[j] = e0 | d << 16;
    for (uint32_t k = 0; k < d; ++k) {
      t.erow[e0 + k] = e0 | d << 16 | k << 24;
      t.ci[e0 + k] = (uint16_t)ci[e0 + k];
    }
  }
  for (int i = 0; i < N; ++i) {
    const uint32_t k0 = (uint32_t)cp[i], d = (uint32_t)(cp[i + 1] - cp[i]);
    t.cols[i] = k0 | d << 16;
    for (uint32_t k = 0; k < d; ++k) {
      const int32_t e = ce[k0 + k];
      t.ce[k0 + k] = (uint16_t)e;
      t.ecol[2 * (size_t)e] = (uint32_t)i | k << 16;
      t.ecol[2 * (size_t)e + 1] = t.cols[i];
    }
  }
}

int launch_onchip_decode(const OnchipView &g, const DecodeArgs &args, int method, int prec,
                         void *stream, int (*resident)[4], uint32_t *advance_out) {
  *advance_out = 0;
  if (args.B <= 0) return 0;
  if ((method != 0 && method != 1) || prec < 0 || prec > 3) return -2;
  OnchipLayout L;
  if (!onchip_plan(g.M, g.N, g.E, g.dc_max, g.dv_max, method, prec, L)) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (method == 1) {
    int &res = resident[1][prec];
    return prec == 1   ? launch_one<1, 1>(g, args, L, st, res, advance_out)
           : prec == 2 ? launch_one<2, 1>(g, args, L, st, res, advance_out)
           : prec == 3 ? launch_one<3, 1>(g, args, L, st, res, advance_out)
                       : launch_one<0, 1>(g, args, L, st, res, advance_out);
  }
  // min-sum has no transcendentals: the f64 modes are one kernel
  int &res = resident[0][prec == 1 ? 1 : 0];
  return prec == 1 ? launch_one<1, 0>(g, args, L, st, res, advance_out)
                   : launch_one<0, 0>(g, args, L, st, res, advance_out);
}

}  // namespace ldpc
