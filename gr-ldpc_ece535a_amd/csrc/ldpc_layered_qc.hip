// ldpc_layered_qc.hip -- layered normalized min-sum for quasi-cyclic codes on
// gfx950 (MI355X), decoded by their block rows: one frame per persistent
// workgroup, the frame's posteriors LQ[N] and check messages R[E] in LDS, as
// in ldpc_layered.hip, whose contract (the header comment there, DESIGN
// section 7b), frame queue, inputs and outputs this kernel keeps bit for bit;
// the per-frame prologue, exit rule and epilogue are the same code
// (ldpc_layered_dev.hpp).  (The reference has neither a layered schedule nor
// structured codes: lib/ldpc_decoder_cb_impl.cc:309-412 is flooding min-sum on
// one dense 32x64 H.)
//
// What a circulant structure (ldpc_qc.hpp) changes is the inside of a layer.
// Layer r is block row r; thread i < Z owns row r * Z + i, threads past Z idle
// up to the layer's barrier.  The row's k-th edge is at column
//   c_k * Z + (i + s_k) mod Z  =  c_k * Z + min(t, t - Z),  t = i + s_k
// (unsigned: t - Z wraps above t where t < Z), with (c_k, s_k) and the degree
// d_r the same for the whole workgroup: one word per base entry, read through
// a uniform pointer (scalar loads, the degree and the first eight entries of a
// block row in one batch), where the table kernel reads a 16-bit column per
// edge from LDS and can issue the LQ read only once that has returned.  R is
// kept place-major within the block row, R[(eb_r + k) * Z + i]
// (eb_r: the base entries before row r), so consecutive lanes touch
// consecutive reals of R and, up to the wrap, of LQ.  The layout is internal:
// within a row ascending block column is ascending column, so place k is the
// contract's k-th edge and every value is the contract's.
//
// The degree is uniform over a layer, so every loop over places has a uniform
// trip count.  Rows of at most 8 places, and of 9 to 16, are gathered whole
// into registers (places past d read some column of the code and place 0 of R,
// and hold +inf); longer rows (up to 32) take two passes over their places.  The leave-one-out minimum is
// the smaller of the row's two smallest |q|, the second at the place of the
// first, as in ldpc_layered.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ldpc_layered.hpp"
#include "ldpc_layered_dev.hpp"
#include "ldpc_qc.hpp"

namespace ldpc {
namespace {

constexpr int kQcRegsShort = 8, kQcRegsLong = 16;
static_assert(kQcRegsLong <= kQcEntPad, "a register row is loaded whole from any entry");

// The base tables are written before the launch and never during it: read
// through the constant address space, a uniform index is a scalar load
// whatever the kernel stores in between (a plain global pointer makes them
// vector loads here, since the frames' outputs might alias it).
typedef const uint32_t __attribute__((address_space(4))) *QcWords;
__device__ __forceinline__ QcWords qc_words(const uint32_t *p) {
  return (QcWords)(uintptr_t)p;
}

// Column of lane i's edge in the circulant w = c * Z | s << 16.
__device__ __forceinline__ int qc_col(uint32_t w, int i, int Z) {
  const uint32_t t = (uint32_t)i + (w >> 16);
  return (int)((w & 0xffffu) + min(t, t - (uint32_t)Z));
}

// One row of d <= D places, whole in registers: w its base entries, Rr its
// first check message (place k at Rr[k * Z]).  The caller loads all D words
// whatever d is: one batch of scalar loads and one wait (a load per place under
// `k < d` compiles to a wait per place).  The words past d are other entries of
// the table or its padding, so their columns are columns of the code, and what
// is read there is replaced by +inf.
template <typename Real, int D>
__device__ __forceinline__ void qc_row_regs(const uint32_t (&w)[D], int d, int Z, int i, Real *LQ,
                                            Real *Rr, Real scale) {
  int c[D];
  Real q[D];
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = qc_col(w[k], i, Z);
  // both operands of every place first: one batch of LDS reads in flight
  Real rv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = LQ[c[k]];
#pragma unroll
  for (int k = 0; k < D; ++k) rv[k] = Rr[(k < d ? k : 0) * Z];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = k < d ? q[k] - rv[k] : (Real)INFINITY;
  // the sign product, the two smallest |q| and the place of the smallest; a
  // place that holds +inf leaves all four as they are
  int P = 1, at = -1;
  Real m1 = Lim<Real>::big(), m2 = Lim<Real>::big();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    P *= ly_sgn(q[k]);
    const Real v = Lim<Real>::abs_(q[k]);
    const bool first = v < m1, second = v < m2;
    m2 = first ? m1 : second ? v : m2;
    m1 = first ? v : m1;
    at = first ? k : at;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (k < d) {
      const Real lo = k == at ? m2 : m1;
      const Real m = scale * ((Real)(P * ly_sgn(q[k])) * lo);
      Rr[k * Z] = m;
      LQ[c[k]] = q[k] + m;
    }
  }
}

// A longer row: the scan, then q_k again (the same operands, the same bits)
// and the row's writes.
template <typename Real>
__device__ __forceinline__ void qc_row_loop(QcWords ent, int d, int Z, int i, Real *LQ,
                                            Real *Rr, Real scale) {
  int P = 1, at = -1;
  Real m1 = Lim<Real>::big(), m2 = Lim<Real>::big();
#pragma unroll 4
  for (int k = 0; k < d; ++k) {
    const Real q = LQ[qc_col(ent[k], i, Z)] - Rr[k * Z];
    P *= ly_sgn(q);
    const Real v = Lim<Real>::abs_(q);
    const bool first = v < m1, second = v < m2;
    m2 = first ? m1 : second ? v : m2;
    m1 = first ? v : m1;
    at = first ? k : at;
  }
#pragma unroll 4
  for (int k = 0; k < d; ++k) {
    const int c = qc_col(ent[k], i, Z);
    const Real q = LQ[c] - Rr[k * Z];
    const Real lo = k == at ? m2 : m1;
    const Real m = scale * ((Real)(P * ly_sgn(q)) * lo);
    Rr[k * Z] = m;
    LQ[c] = q + m;
  }
}

// Syndrome weight of the decisions LQ < 0 (checkFrame :236-253, no
// threshold), block row by block row: thread i XORs the decisions at its row's
// places, a ballot per block row counts the odd ones, and every thread gets
// the sum.  Four block rows go side by side: their records, then their first
// eight entries, then their LQ reads are each one batch; one block row at a
// time is a scalar and an LDS round trip per block row, with nothing else to
// run on a one-wave workgroup.  Threads past Z read lane Z - 1's columns and
// are left out of the ballot, so the reads sit in no branch.
constexpr int kQcSynRows = 4;

template <typename Real>
__device__ __forceinline__ int qc_syndrome(const LayeredQcView &g, const Real *LQ, int *red) {
  const int tid = threadIdx.x, Z = g.Z;
  const int i = min(tid, Z - 1);
  const bool mine = tid < Z;
  int cnt = 0;
  for (int r0 = 0; r0 < g.mb; r0 += kQcSynRows) {  // every wave sees every ballot
    int d[kQcSynRows];
    QcWords ent[kQcSynRows];
    uint32_t w[kQcSynRows][kQcRegsShort];
#pragma unroll
    for (int s = 0; s < kQcSynRows; ++s) {
      const bool ok = r0 + s < g.mb;
      const uint32_t rec = qc_words(g.rows)[ok ? r0 + s : 0];
      d[s] = ok ? (int)(rec & 0xffffu) : 0;
      ent[s] = qc_words(g.ent) + (rec >> 16);
    }
#pragma unroll
    for (int s = 0; s < kQcSynRows; ++s)
#pragma unroll
      for (int k = 0; k < kQcRegsShort; ++k) w[s][k] = ent[s][k];
    bool odd[kQcSynRows];
#pragma unroll
    for (int s = 0; s < kQcSynRows; ++s) {
      odd[s] = false;
#pragma unroll
      for (int k = 0; k < kQcRegsShort; ++k)
        odd[s] ^= (LQ[qc_col(w[s][k], i, Z)] < Real(0)) & (k < d[s]);
    }
#pragma unroll
    for (int s = 0; s < kQcSynRows; ++s)
      for (int k = kQcRegsShort; k < d[s]; ++k) odd[s] ^= LQ[qc_col(ent[s][k], i, Z)] < Real(0);
#pragma unroll
    for (int s = 0; s < kQcSynRows; ++s) cnt += __popcll(__ballot(odd[s] & mine));
  }
  return ly_sum_waves(cnt, red);
}

template <typename Real>
__global__ void __launch_bounds__(kLayeredMaxThreads)
    layered_qc_decode_kernel(LayeredQcView gv, DecodeArgs a, LayeredLayout lay, Real scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  Real *LQ = reinterpret_cast<Real *>(smem);
  Real *R = reinterpret_cast<Real *>(smem + lay.r);
  uint8_t *hard = smem + lay.hard;
  int *red = reinterpret_cast<int *>(smem + lay.red);
  const int tid = threadIdx.x;
  const int M = gv.M, N = gv.N, E = gv.E, Z = gv.Z, mb = gv.mb;

  int64_t b = blockIdx.x;
  while (b < a.B) {
    ly_load_frame(a, b, N, E, LQ, R);
    int used = 0, weight = 0;
    for (int h = 0;; ++h) {
      int eb = 0;  // the base entries before block row r: a running sum, so that
                   // the row's degree and its first entries load side by side
      for (int r = 0; r < mb; ++r) {
        QcWords ent = qc_words(gv.ent) + eb;
        const int d = (int)(qc_words(gv.rows)[r] & 0xffffu);
        __builtin_assume(d >= 1);  // the table lists no empty block row
        uint32_t w[kQcRegsLong];
#pragma unroll
        for (int k = 0; k < kQcRegsShort; ++k) w[k] = ent[k];
        if (tid < Z) {
          Real *Rr = R + eb * Z + tid;
          if (d <= kQcRegsShort) {
            const uint32_t(&w8)[kQcRegsShort] = reinterpret_cast<const uint32_t(&)[kQcRegsShort]>(w);
            qc_row_regs<Real, kQcRegsShort>(w8, d, Z, tid, LQ, Rr, scale);
          } else if (d <= kQcRegsLong) {
#pragma unroll
            for (int k = kQcRegsShort; k < kQcRegsLong; ++k) w[k] = ent[k];
            qc_row_regs<Real, kQcRegsLong>(w, d, Z, tid, LQ, Rr, scale);
          } else {
            qc_row_loop(ent, d, Z, tid, LQ, Rr, scale);
          }
        }
        __syncthreads();
        eb += d;
      }
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period (:406-408)
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        weight = qc_syndrome(gv, LQ, red);
        if (last || weight == 0) break;
      }
    }
    ly_store_frame(a, b, M, N, gv.KB, used, weight, LQ, hard);
    b = ly_next_frame(a, b, red);
  }
}

template <typename Real>
int launch_kernel(const LayeredQcView &g, DecodeArgs a, const LayeredLayout &lay, double scale,
                  hipStream_t st, int &resident) {
  const void *fn = (const void *)layered_qc_decode_kernel<Real>;
  if (!ly_resident(fn, lay.threads, lay.total, resident)) return -3;
  a.waves = (int)std::min<int64_t>(a.B, resident);
  hipLaunchKernelGGL((layered_qc_decode_kernel<Real>), dim3((unsigned)a.waves),
                     dim3((unsigned)lay.threads), (size_t)lay.total, st, g, a, lay, (Real)scale);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int launch_layered_qc_decode(const LayeredQcView &g, const DecodeArgs &args,
                             const LayeredLayout &lay, double scale, int prec, void *stream,
                             int *resident, uint32_t *advance_out) {
  *advance_out = 0;
  if (args.B <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int rc = prec == 1 ? launch_kernel<float>(g, args, lay, scale, st, resident[1])
                           : launch_kernel<double>(g, args, lay, scale, st, resident[0]);
  // one add per frame decoded, each workgroup's last being the one past the batch
  if (rc == 0 && !args.static_stride) *advance_out = (uint32_t)args.B;
  return rc;
}

}  // namespace ldpc
