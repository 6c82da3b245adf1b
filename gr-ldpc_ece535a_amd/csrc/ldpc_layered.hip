// ldpc_layered.hip -- layered (row-serial) normalized min-sum for gfx950
// (MI355X): one frame per persistent workgroup, the frame's posteriors LQ[N]
// and check messages R[E] in LDS from the first iteration to the last.
//
// The reference has only the flooding schedule and plain min-sum in double on
// one dense 32x64 H (lib/ldpc_decoder_cb_impl.cc:309-412): it has neither a
// layered schedule, nor structured codes, nor fixed point.  This decoder keeps
// its conventions (Lci = -tx, decision LQ < 0, min-sum's exit rule :406-408)
// and changes the schedule: the rows of H are taken layer by layer
// (ldpc_layers.hpp), each row reading the posteriors the rows before it have
// already updated, and every check message is normalised.  Per row j with
// edges e_0..e_{d-1} in ascending column c_0 < ... < c_{d-1}:
//
//   q_k  = LQ[c_k] - R[e_k]
//   lo_k = min(seed, |q_t| for t != k)
//   R[e_k]  = the normalised lo_k under the sign of the other places' q
//   LQ[c_k] = q_k + R[e_k]
//
// A thread owns a row of the current layer.  The rows of a layer share no
// column, so a thread's LQ and R cells are its own until the barrier that ends
// the layer.  The leave-one-out minimum is the smaller of the row's two
// smallest |q| (the second where k is the place of the first): the same value,
// hence the same bits, as the scan over t != k.
//
// Nine kernels are one template (layered_kernel) over two choices that share
// everything else (and nine more with a third, the frame load: load_frame for
// N samples in column order, load_frame_rm for rate-matched samples; and each
// of the eighteen once more with the code-block CRC of ldpc_crc.hpp checked
// beside the syndrome): an
// arithmetic (FloatArith<double / float>, Q8Arith: the
// types, the row's scan and message, a sample's load, the decisions) and a
// route (TableRoute<staged / L2>, CirculantRoute: the tables, which rows a
// thread runs in a layer and where their columns and messages are, the
// syndrome).  What surrounds them -- a sample's Lci, the workgroup's
// reduction words, a frame's outputs, the frame queue -- is in
// ldpc_wgframe.hpp, shared with the on-chip flooding kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <type_traits>

#include "ldpc_dispatch.hpp"
#include "ldpc_layered.hpp"
#include "ldpc_qc.hpp"
#include "ldpc_wgframe.hpp"

namespace ldpc {
namespace {

// ---- the arithmetics -------------------------------------------------------------

// The float contract (include/ldpc_hip.h), Real = double or
// float, a = scale:
//
//   LQ[i] = (Real)Lci_i;  R[e] = 0
//   s_k  = sign(q_k) (sign(0) = 0), P = s_0 * ... * s_{d-1}
//   lo_k = min(BIG, |q_t| for t != k)          (strict <: NaN and inf never win;
//                                               BIG = DBL_MAX / FLT_MAX, the reference's seed)
//   R[e_k]  = a * ((Real)(P * s_k) * lo_k)     (only the multiply by a rounds)
//
// No arithmetic here contracts (-ffp-contract=off) and none is transcendental,
// so the f64 precisions are one kernel.  The decisions LQ < 0 are taken once
// per frame into hard[N] behind R, which the epilogue reads.
template <typename Real>
struct FloatArith {
  using Post = Real;  // LQ
  using Msg = Real;   // R
  using Reg = Real;   // a q in registers
  using Par = bool;   // a row's parity of decisions
  static constexpr bool kHardRegion = true;
  Real scale;

  // what a place past the row's degree holds: sign +, never below a minimum
  static __device__ __forceinline__ Reg pad() { return (Real)INFINITY; }
  static __device__ __forceinline__ int sgn(Real v) { return (v > Real(0)) - (v < Real(0)); }

  // the sign product, the two smallest |q| and the place of the smallest
  struct Row {
    int P = 1, at = -1;
    Real m1 = std::numeric_limits<Real>::max(), m2 = std::numeric_limits<Real>::max();
  };
  static __device__ __forceinline__ void scan(Row &s, Real q, int k) {
    s.P *= sgn(q);
    const Real v = __builtin_elementwise_abs(q);
    const bool first = v < s.m1, second = v < s.m2;
    s.m2 = first ? s.m1 : second ? v : s.m2;
    s.m1 = first ? v : s.m1;
    s.at = first ? k : s.at;
  }
  __device__ __forceinline__ Real msg(const Row &s, Real q, int k) const {
    const Real lo = k == s.at ? s.m2 : s.m1;
    return scale * ((Real)(s.P * sgn(q)) * lo);
  }

  __device__ __forceinline__ Post sample(float lci) const { return (Real)lci; }
  static __device__ __forceinline__ void clear(Msg *R, int E, const LayeredLayout &) {
    for (int e = threadIdx.x; e < E; e += blockDim.x) R[e] = Real(0);
  }
  static __device__ __forceinline__ bool decision(Post v) { return v < Real(0); }
  static __device__ __forceinline__ Par term(Post v) { return v < Real(0); }
  static __device__ __forceinline__ bool odd(Par x) { return x; }
};

// The fixed-point contract (include/ldpc_hip.h), num in
// [1, 16]: the check messages R[E] are int8 and the posteriors LQ[N] int16, so a
// frame is a16(2 N) + a16(E) + 128 bytes where the float layouts need 5 N + 4 E.
//
//   v_i = Lci_i * llr_scale                                      (float)
//   LQ[i] = v_i is NaN ? 0 : clamp(rint(v_i), -127, 127);  R[e] = 0
//   s_k  = q_k < 0 ? -1 : +1,  P = s_0 * ... * s_{d-1}
//   lo_k = min(127, |q_t| for t != k)
//   R[e_k]  = (P * s_k) * ((lo_k * num + 8) >> 4)
//
// All of it is integer arithmetic in 32-bit registers; what is stored fits its
// type exactly: |R| <= 127, and LQ[c] = Lc_c + the sum of the column's R after
// every update, so |LQ| <= 127 (dv + 1) <= 32767 (layered_q8_layout checks dv).
// The sign product is the XOR of the q's sign bits.  The decisions are LQ < 0,
// read in place: there is no decision array.  Consecutive lanes of the
// circulant route touch consecutive bytes of R and, up to the wrap, consecutive
// halfwords of LQ: four and two lanes to a dword.
struct Q8Arith {
  using Post = int16_t;
  using Msg = int8_t;
  using Reg = int;
  using Par = int;  // the XOR of a row's posteriors: its sign is the parity
  static constexpr bool kHardRegion = false;
  static constexpr int kMax = 127;
  int num;
  float llr_scale;

  static __device__ __forceinline__ Reg pad() { return 32767; }

  // The XOR of the q's (its sign bit is that of P), the two smallest |q| below
  // the seed and the place of the smallest.
  struct Row {
    int sg = 0, m1 = kMax, m2 = kMax, at = -1;
  };
  static __device__ __forceinline__ void scan(Row &s, int q, int k) {
    s.sg ^= q;
    const int v = q < 0 ? -q : q;
    const bool first = v < s.m1, second = v < s.m2;
    s.m2 = first ? s.m1 : second ? v : s.m2;
    s.m1 = first ? v : s.m1;
    s.at = first ? k : s.at;
  }
  __device__ __forceinline__ int msg(const Row &s, int q, int k) const {
    const int lo = k == s.at ? s.m2 : s.m1;
    const int mag = (lo * num + 8) >> 4;
    return (s.sg ^ q) < 0 ? -mag : mag;
  }

  __device__ __forceinline__ Post sample(float lci) const {
    const float v = lci * llr_scale;
    const float c = fminf(fmaxf(rintf(v), -(float)kMax), (float)kMax);
    return v != v ? (int16_t)0 : (int16_t)(int)c;
  }
  // as dwords: R's region is a multiple of 16 bytes
  static __device__ __forceinline__ void clear(Msg *R, int, const LayeredLayout &lay) {
    uint32_t *R32 = reinterpret_cast<uint32_t *>(R);
    const int n = (lay.red - lay.r) >> 2;
    for (int e = threadIdx.x; e < n; e += blockDim.x) R32[e] = 0u;
  }
  static __device__ __forceinline__ bool decision(Post v) { return v < 0; }
  static __device__ __forceinline__ Par term(Post v) { return v; }
  static __device__ __forceinline__ bool odd(Par x) { return x < 0; }
};

// ---- the row update --------------------------------------------------------------

// Rows of at most D places are gathered whole into registers: the row's columns
// in one batch of independent reads, both operands of every place in a second,
// where a loop over the places would wait for each read in turn (DESIGN section
// 7a: such chains are what the on-chip kernels' time is).  Places past d read
// some column of the code (col_pad) and the message of place 0, and hold
// Arith::pad(), which leaves the scan's state as it is, so the scan has no
// branches.  Rr: the row's first message; Addr: where place k's column (col)
// and message (Rr[msg(k)]) are.
template <int D, typename Arith, typename Addr>
__device__ __forceinline__ void row_regs(const Arith &ar, const Addr &ad, int d,
                                         typename Arith::Post *LQ, typename Arith::Msg *Rr) {
  using Reg = typename Arith::Reg;
  int c[D];
  Reg q[D], rv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = ad.col_pad(k, d);
  // the messages first: their addresses need no column, so on the table
  // route they are in flight while the column indices arrive
#pragma unroll
  for (int k = 0; k < D; ++k) rv[k] = Rr[ad.msg(k < d ? k : 0)];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = LQ[c[k]];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = k < d ? q[k] - rv[k] : Arith::pad();
  typename Arith::Row s;
#pragma unroll
  for (int k = 0; k < D; ++k) Arith::scan(s, q[k], k);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (k < d) {
      const Reg m = ar.msg(s, q[k], k);
      Rr[ad.msg(k)] = (typename Arith::Msg)m;
      LQ[c[k]] = (typename Arith::Post)(q[k] + m);
    }
  }
}

// A longer row: the scan, then q_k again (the same operands, the same bits)
// and the row's writes.
template <typename Arith, typename Addr>
__device__ __forceinline__ void row_loop(const Arith &ar, const Addr &ad, int d,
                                         typename Arith::Post *LQ, typename Arith::Msg *Rr) {
  using Reg = typename Arith::Reg;
  typename Arith::Row s;
#pragma unroll 4
  for (int k = 0; k < d; ++k) Arith::scan(s, (Reg)LQ[ad.col(k)] - (Reg)Rr[ad.msg(k)], k);
#pragma unroll 4
  for (int k = 0; k < d; ++k) {
    const int c = ad.col(k);
    const Reg q = (Reg)LQ[c] - (Reg)Rr[ad.msg(k)];
    const Reg m = ar.msg(s, q, k);
    Rr[ad.msg(k)] = (typename Arith::Msg)m;
    LQ[c] = (typename Arith::Post)(q + m);
  }
}

// ---- the table route -------------------------------------------------------------

constexpr int kRegsShort = 8, kRegsLong = 16;
static_assert(kRegsLong <= kQcEntPad, "a register row is loaded whole from any entry");

// A row of the per-edge tables: ci its first column index, its messages at Rr[k].
struct TabAddr {
  const uint16_t *ci;
  __device__ __forceinline__ int col(int k) const { return ci[k]; }
  __device__ __forceinline__ int col_pad(int k, int d) const { return ci[k < d ? k : 0]; }
  __device__ __forceinline__ int msg(int k) const { return k; }
};

// Any plan through per-edge tables (LayeredTables): a thread per row of the
// layer, rows of at most 8 places in registers and longer ones (up to 32) in
// two passes.  STAGED: the tables fit behind the frame and are copied to LDS
// once per launch; otherwise they are read from global memory (L2).
template <bool STAGED>
struct TableRoute {
  using View = LayeredView;
  const uint32_t *rows;
  const uint16_t *ci;
  const uint16_t *order;
  const uint32_t *off;
  int M, L;

  __device__ __forceinline__ void init(const View &gv, unsigned char *smem,
                                       const LayeredLayout &lay) {
    M = gv.M;
    L = gv.L;
    rows = gv.rows;
    ci = gv.ci;
    order = gv.order;
    off = gv.off;
    if constexpr (STAGED) {
      uint32_t *s_rows = reinterpret_cast<uint32_t *>(smem + lay.rows);
      uint16_t *s_ci = reinterpret_cast<uint16_t *>(smem + lay.ci);
      uint16_t *s_order = reinterpret_cast<uint16_t *>(smem + lay.order);
      uint32_t *s_off = reinterpret_cast<uint32_t *>(smem + lay.off);
      wg_copy(s_rows, gv.rows, M);
      wg_copy(s_ci, gv.ci, gv.E);
      wg_copy(s_order, gv.order, M);
      wg_copy(s_off, gv.off, L + 1);
      rows = s_rows;
      ci = s_ci;
      order = s_order;
      off = s_off;
      __syncthreads();
    }
  }
  __device__ __forceinline__ int layers() const { return L; }
  __device__ __forceinline__ void rewind() {}

  template <typename Arith>
  __device__ __forceinline__ void run_layer(int l, const Arith &ar, typename Arith::Post *LQ,
                                            typename Arith::Msg *R) {
    const int r1 = (int)off[l + 1];
    for (int r = (int)off[l] + threadIdx.x; r < r1; r += blockDim.x) {
      const uint32_t rec = rows[order[r]];
      const int e0 = rec & 0xffff, d = rec >> 16;
      const TabAddr ad{ci + e0};
      if (d > 0 && d <= kRegsShort)
        row_regs<kRegsShort>(ar, ad, d, LQ, R + e0);
      else
        row_loop(ar, ad, d, LQ, R + e0);
    }
  }

  // Syndrome weight of the decisions (checkFrame :236-253, no threshold), read
  // from the posteriors in LDS: every thread gets the sum.
  template <typename Arith>
  __device__ __forceinline__ int syndrome(const typename Arith::Post *LQ, int *red) const {
    using Par = typename Arith::Par;
    const int tid = threadIdx.x, T = blockDim.x;
    int cnt = 0;
    for (int j0 = 0; j0 < M; j0 += T) {  // uniform trip count: the ballots see whole waves
      const int j = j0 + tid;
      Par x = Par(0);
      if (j < M) {
        const uint32_t rec = rows[j];
        const int e0 = rec & 0xffff, d = rec >> 16;
        if (d > 0 && d <= kRegsShort) {
          // every place is read, in one batch; a read under `k < d` is a
          // branch and a wait per place
          int c[kRegsShort];
          Par v[kRegsShort];
#pragma unroll
          for (int k = 0; k < kRegsShort; ++k) c[k] = ci[e0 + (k < d ? k : 0)];
#pragma unroll
          for (int k = 0; k < kRegsShort; ++k) v[k] = Arith::term(LQ[c[k]]);
#pragma unroll
          for (int k = 0; k < kRegsShort; ++k) x ^= k < d ? v[k] : Par(0);
        } else {
          for (int t = 0; t < d; ++t) x ^= Arith::term(LQ[ci[e0 + t]]);
        }
      }
      cnt += __popcll(__ballot(Arith::odd(x)));
    }
    return wg_sum_waves(cnt, red);
  }
};

// ---- the circulant route ---------------------------------------------------------

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

// Lane i's row of a block row: place k's column from the entry word w[k] (W:
// registers or the table itself), its message at Rr[k * Z].  The words past d
// are other entries of the table or its padding, so their columns are columns
// of the code.
template <typename W>
struct QcAddr {
  W w;
  int i, Z;
  __device__ __forceinline__ int col(int k) const { return qc_col(w[k], i, Z); }
  __device__ __forceinline__ int col_pad(int k, int) const { return col(k); }
  __device__ __forceinline__ int msg(int k) const { return k * Z; }
};

// A quasi-cyclic code (ldpc_qc.hpp) decoded by its block rows.  Layer r is
// block row r; thread i < Z owns row r * Z + i, threads past Z idle up to the
// layer's barrier.  The row's k-th edge is at column
//   c_k * Z + (i + s_k) mod Z  =  c_k * Z + min(t, t - Z),  t = i + s_k
// (unsigned: t - Z wraps above t where t < Z), with (c_k, s_k) and the degree
// d_r the same for the whole workgroup: one word per base entry, read through
// a uniform pointer (scalar loads, the degree and the first eight entries of a
// block row in one batch), where the table route reads a 16-bit column per
// edge and can issue the LQ read only once that has returned.  R is kept
// place-major within the block row, R[(eb_r + k) * Z + i] (eb_r: the base
// entries before row r), so consecutive lanes touch consecutive cells of R
// and, up to the wrap, of LQ.  The layout is internal: within a row ascending
// block column is ascending column, so place k is the contract's k-th edge and
// every value is the contract's.
//
// The degree is uniform over a layer, so every loop over places has a uniform
// trip count.  Rows of at most 8 places, and of 9 to 16, are gathered whole
// into registers; longer rows (up to 32) take two passes over their places.
struct CirculantRoute {
  using View = LayeredQcView;
  QcWords rows, ent;
  int mb, Z;
  int eb;  // the base entries before the next block row: a running sum, so that
           // the row's degree and its first entries load side by side

  __device__ __forceinline__ void init(const View &gv, unsigned char *, const LayeredLayout &) {
    rows = qc_words(gv.rows);
    ent = qc_words(gv.ent);
    mb = gv.mb;
    Z = gv.Z;
  }
  __device__ __forceinline__ int layers() const { return mb; }
  __device__ __forceinline__ void rewind() { eb = 0; }

  template <typename Arith>
  __device__ __forceinline__ void run_layer(int r, const Arith &ar, typename Arith::Post *LQ,
                                            typename Arith::Msg *R) {
    const int tid = threadIdx.x;
    QcWords e = ent + eb;
    const int d = (int)(rows[r] & 0xffffu);
    __builtin_assume(d >= 1);  // the table lists no empty block row
    // The first eight words whatever d is: one batch of scalar loads and one
    // wait (a load per place under `k < d` compiles to a wait per place).
    uint32_t w[kRegsLong];
#pragma unroll
    for (int k = 0; k < kRegsShort; ++k) w[k] = e[k];
    if (tid < Z) {
      typename Arith::Msg *Rr = R + eb * Z + tid;
      if (d <= kRegsShort) {
        row_regs<kRegsShort>(ar, QcAddr<const uint32_t *>{w, tid, Z}, d, LQ, Rr);
      } else if (d <= kRegsLong) {
#pragma unroll
        for (int k = kRegsShort; k < kRegsLong; ++k) w[k] = e[k];
        row_regs<kRegsLong>(ar, QcAddr<const uint32_t *>{w, tid, Z}, d, LQ, Rr);
      } else {
        row_loop(ar, QcAddr<QcWords>{e, tid, Z}, d, LQ, Rr);
      }
    }
    eb += d;
  }

  // Syndrome weight of the decisions (checkFrame :236-253, no threshold), block
  // row by block row: thread i combines the decisions at its row's places, a
  // ballot per block row counts the odd ones, and every thread gets the sum.
  // Four block rows go side by side: their records, then their first eight
  // entries, then their LQ reads are each one batch; one block row at a time
  // is a scalar and an LDS round trip per block row, with nothing else to run
  // on a one-wave workgroup.  Threads past Z read lane Z - 1's columns and are
  // left out of the ballot, so the reads sit in no branch.
  static constexpr int kSynRows = 4;

  template <typename Arith>
  __device__ __forceinline__ int syndrome(const typename Arith::Post *LQ, int *red) const {
    using Par = typename Arith::Par;
    const int tid = threadIdx.x;
    const int i = min(tid, Z - 1);
    const bool mine = tid < Z;
    int cnt = 0;
    for (int r0 = 0; r0 < mb; r0 += kSynRows) {  // every wave sees every ballot
      int d[kSynRows];
      QcWords e[kSynRows];
      uint32_t w[kSynRows][kRegsShort];
#pragma unroll
      for (int s = 0; s < kSynRows; ++s) {
        const bool ok = r0 + s < mb;
        const uint32_t rec = rows[ok ? r0 + s : 0];
        d[s] = ok ? (int)(rec & 0xffffu) : 0;
        e[s] = ent + (rec >> 16);
      }
#pragma unroll
      for (int s = 0; s < kSynRows; ++s)
#pragma unroll
        for (int k = 0; k < kRegsShort; ++k) w[s][k] = e[s][k];
      Par x[kSynRows];
#pragma unroll
      for (int s = 0; s < kSynRows; ++s) {
        x[s] = Par(0);
#pragma unroll
        for (int k = 0; k < kRegsShort; ++k) {
          const Par v = Arith::term(LQ[qc_col(w[s][k], i, Z)]);
          x[s] ^= k < d[s] ? v : Par(0);
        }
      }
#pragma unroll
      for (int s = 0; s < kSynRows; ++s)
        for (int k = kRegsShort; k < d[s]; ++k) x[s] ^= Arith::term(LQ[qc_col(e[s][k], i, Z)]);
#pragma unroll
      for (int s = 0; s < kSynRows; ++s) cnt += __popcll(__ballot(Arith::odd(x[s]) & mine));
    }
    return wg_sum_waves(cnt, red);
  }
};

// ---- a frame ---------------------------------------------------------------------

// Frame b into LDS: LQ = the samples' Lci in the arithmetic's format, R = 0;
// ends with the barrier that lets the first layer read them.  The layered
// entry points take strided frames only (no window lists, no second-polarity
// half: DecodeArgs::win and pm_half are unset), so this is frame_src's last
// line alone; the general case is frame_src (ldpc_wgframe.hpp).
template <typename Arith>
__device__ __forceinline__ void load_frame(const Arith &ar, const DecodeArgs &a, int64_t b, int N,
                                           int E, const LayeredLayout &lay,
                                           typename Arith::Post *LQ, typename Arith::Msg *R) {
  const int tid = threadIdx.x, T = blockDim.x;
  const float pol = a.polarity;
  const float *src = a.in + b * a.cw_stride;
  for (int i = tid; i < N; i += T) LQ[i] = ar.sample(lci_of(src[(int64_t)i * a.elem_stride], pol));
  Arith::clear(R, E, lay);
  __syncthreads();
}

// The same for a frame of rate-matched samples (ldpc_rate_match.hpp): the
// frame is what its transmissions hold, at a.in + b * a.cw_stride, and every
// column gathers its own terms -- the first sample of each transmission that
// lands on it, then steps of S -- and adds them in that order.  A thread
// strides over the columns; consecutive columns read consecutive samples up to
// the buffer's wrap and the fillers.  No LDS beyond the frame, no atomics, and
// the barrier that ends the load is still the only one.  (Fetching the first
// terms of eight columns side by side, and the per-transmission words at
// constant indices, were both measured and both lost to this loop:
// profiles/round21/rate_match_ab_batched.txt, rate_match_ab_unrolled.txt.)
template <typename Arith>
__device__ __forceinline__ void load_frame_rm(const Arith &ar, const DecodeArgs &a,
                                              const RmArgs &rm, int64_t b, int N, int E,
                                              const LayeredLayout &lay, typename Arith::Post *LQ,
                                              typename Arith::Msg *R) {
  const int tid = threadIdx.x, T = blockDim.x;
  const float pol = a.polarity;
  const float *src = a.in + b * a.cw_stride;
  for (int i = tid; i < N; i += T)
    LQ[i] = ar.sample(rm_column_lci(rm, i, [&](int k) { return lci_term_of(src[k], pol); }));
  Arith::clear(R, E, lay);
  __syncthreads();
}

// Frame b's outputs (the syndrome's barrier is behind every LQ write): the
// decisions into hard[N] where the arithmetic keeps them, then wg_store_frame.
template <typename Arith>
__device__ __forceinline__ void store_frame(const DecodeArgs &a, int64_t b, int M, int N, int KB,
                                            int used, int weight, const typename Arith::Post *LQ,
                                            uint8_t *hard) {
  const int tid = threadIdx.x, T = blockDim.x;
  if constexpr (Arith::kHardRegion) {
    for (int i = tid; i < N; i += T) hard[i] = Arith::decision(LQ[i]);
    __syncthreads();
  }
  const auto bit = [&](int i) -> uint32_t {
    if constexpr (Arith::kHardRegion)
      return hard[i];
    else
      return Arith::decision(LQ[i]);
  };
  wg_store_frame(a, b, M, N, KB, used, weight, bit, [&](int i) { return (float)LQ[i]; });
}

// ---- the code-block CRC ----------------------------------------------------------

// The kernel's trailing arguments, by type: an RmArgs, a CrcArgs, both in that
// order, or neither.
template <typename... X>
constexpr bool kHasRm = (std::is_same_v<X, RmArgs> || ...);
template <typename... X>
constexpr bool kHasCrc = (std::is_same_v<X, CrcArgs> || ...);
template <typename... X>
__device__ __forceinline__ const RmArgs &rm_of(const RmArgs &rm, const X &...) {
  return rm;
}
__device__ __forceinline__ const CrcArgs &crc_of(const CrcArgs &c) { return c; }
__device__ __forceinline__ const CrcArgs &crc_of(const RmArgs &, const CrcArgs &c) { return c; }

// A wave's share of the block's remainder (ldpc_crc.hpp) into the workgroup's
// CRC bytes: the XOR of w[p] over the block positions p whose decision is 1,
// the workgroup's threads striding over p and selecting with a mask, folded
// over the wave's lanes.  The posteriors are read where they are, in LDS; the
// weights through the constant address space (written before the launch,
// never during it).  No barrier: the syndrome's, which follows, is behind
// these writes, and the next check's writes are behind a layer's.
//
// (Eight strides' reads batched side by side and the wave folded through DPP
// and four lane reads was measured and did not beat this loop:
// profiles/round22/crc_ab_batched.txt.  The loop is not unrolled: unrolled by
// the compiler the batched form spilled some 200 registers.)
template <typename Arith>
__device__ __forceinline__ void crc_wave_share(const CrcArgs &c, const typename Arith::Post *LQ,
                                               int *red) {
  const int tid = threadIdx.x, T = blockDim.x;
  QcWords w = qc_words(c.w);
  const typename Arith::Post *info = LQ + c.M;
  uint32_t x = 0;
#pragma unroll 1
  for (int p = tid; p < c.A; p += T) x ^= w[p] & (0u - (uint32_t)Arith::decision(info[p]));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x ^= (uint32_t)__shfl_xor((int)x, m, 64);
  if ((tid & 63) == 0) {
    uint8_t *by = reinterpret_cast<uint8_t *>(red + kWgRedCrc) + 3 * (tid >> 6);
    by[0] = (uint8_t)x;
    by[1] = (uint8_t)(x >> 8);
    by[2] = (uint8_t)(x >> 16);
  }
}

// The workgroup's remainder from its CRC bytes, behind a barrier: every thread
// gets it.  Sixteen 3-byte records in twelve words, those of absent waves zero
// since the launch: the words are folded four records at a time, then the four.
__device__ __forceinline__ uint32_t crc_remainder(const int *red) {
  const uint32_t *v = reinterpret_cast<const uint32_t *>(red + kWgRedCrc);
  uint32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
  for (int j = 0; j < kWgRedCrcWords; j += 3) {
    a0 ^= v[j];
    a1 ^= v[j + 1];
    a2 ^= v[j + 2];
  }
  return (a0 & 0xffffffu) ^ ((a0 >> 24) | ((a1 & 0xffffu) << 8)) ^
         ((a1 >> 16) | ((a2 & 0xffu) << 16)) ^ (a2 >> 8);
}

// Rm: nothing (the frames are N samples in column order: load_frame), one
// RmArgs (the frames are rate-matched samples: load_frame_rm), one CrcArgs
// (the block's remainder is checked beside the syndrome and stored with the
// frame), or an RmArgs and a CrcArgs.
template <typename Arith, typename Route, typename... Rm>
__global__ void __launch_bounds__(kLayeredMaxThreads)
    layered_kernel(typename Route::View gv, DecodeArgs a, LayeredLayout lay, Arith ar, Rm... rm) {
  using Post = typename Arith::Post;
  using Msg = typename Arith::Msg;
  extern __shared__ __align__(16) unsigned char smem[];
  Post *LQ = reinterpret_cast<Post *>(smem);
  Msg *R = reinterpret_cast<Msg *>(smem + lay.r);
  uint8_t *hard = smem + lay.hard;
  int *red = reinterpret_cast<int *>(smem + lay.red);
  Route route;
  route.init(gv, smem, lay);
  const int NL = route.layers();
  constexpr bool kRm = kHasRm<Rm...>, kCrc = kHasCrc<Rm...>;
  // the CRC bytes of waves this workgroup does not have stay zero; the first
  // frame's load ends with a barrier
  if constexpr (kCrc)
    if (threadIdx.x < kWgRedCrcWords) red[kWgRedCrc + threadIdx.x] = 0;

  int64_t b = blockIdx.x;
  while (b < a.B) {
    if constexpr (kRm)
      load_frame_rm(ar, a, rm_of(rm...), b, gv.N, gv.E, lay, LQ, R);
    else
      load_frame(ar, a, b, gv.N, gv.E, lay, LQ, R);
    int used = 0, weight = 0;
    [[maybe_unused]] uint32_t rem = 0;
    for (int h = 0;; ++h) {
      route.rewind();
      for (int l = 0; l < NL; ++l) {
        route.run_layer(l, ar, LQ, R);
        __syncthreads();
      }
      used = h + 1;
      // the cap first, then the syndrome on multiples of et_period (:406-408)
      const bool last = used == a.max_iters;
      if (last || used % a.et_period == 0) {
        if constexpr (kCrc) {
          // the remainder of the same decisions, through the syndrome's barrier
          crc_wave_share<Arith>(crc_of(rm...), LQ, red);
          weight = route.template syndrome<Arith>(LQ, red);
          rem = crc_remainder(red);
          if (last || weight == 0 || (crc_of(rm...).stop && rem == 0)) break;
        } else {
          weight = route.template syndrome<Arith>(LQ, red);
          if (last || weight == 0) break;
        }
      }
    }
    if constexpr (kCrc)
      if (threadIdx.x == 0) crc_of(rm...).out[b] = rem;
    store_frame<Arith>(a, b, gv.M, gv.N, gv.KB, used, weight, LQ, hard);
    b = wg_next_frame(a, b, red);
  }
}

// ---- the launch ------------------------------------------------------------------

template <typename Arith, typename Route, typename... Rm>
int launch_kernel(const typename Route::View &g, DecodeArgs a, const LayeredLayout &lay, Arith ar,
                  hipStream_t st, int &resident, uint32_t *advance_out, Rm... rm) {
  if (!wg_launch((const void *)layered_kernel<Arith, Route, Rm...>, lay.threads, lay.total,
                 resident, a, advance_out))
    return -3;
  hipLaunchKernelGGL((layered_kernel<Arith, Route, Rm...>), dim3((unsigned)a.waves),
                     dim3((unsigned)lay.threads), (size_t)lay.total, st, g, a, lay, ar, rm...);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <typename Route, typename... Rm>
int launch_arith(const typename Route::View &g, const DecodeArgs &args, const LayeredLayout &lay,
                 const LayeredArith &ar, hipStream_t st, int *resident, uint32_t *advance_out,
                 Rm... rm) {
  if (ar.kind == kLayeredQ8)
    return launch_kernel<Q8Arith, Route>(g, args, lay, {ar.num, ar.llr_scale}, st, *resident,
                                         advance_out, rm...);
  if (ar.kind == kLayeredF32)
    return launch_kernel<FloatArith<float>, Route>(g, args, lay, {(float)ar.scale}, st, *resident,
                                                   advance_out, rm...);
  return launch_kernel<FloatArith<double>, Route>(g, args, lay, {ar.scale}, st, *resident,
                                                  advance_out, rm...);
}

template <typename Route>
int launch_route(const typename Route::View &g, const DecodeArgs &args, const LayeredLayout &lay,
                 const LayeredArith &ar, void *stream, int *resident, uint32_t *advance_out,
                 const RmArgs *rm, const CrcArgs *crc) {
  *advance_out = 0;
  if (args.B <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (crc)
    return rm ? launch_arith<Route>(g, args, lay, ar, st, resident, advance_out, *rm, *crc)
              : launch_arith<Route>(g, args, lay, ar, st, resident, advance_out, *crc);
  return rm ? launch_arith<Route>(g, args, lay, ar, st, resident, advance_out, *rm)
            : launch_arith<Route>(g, args, lay, ar, st, resident, advance_out);
}

}  // namespace

int launch_layered_decode(const LayeredView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          const LayeredArith &ar, void *stream, int *resident,
                          uint32_t *advance_out, const RmArgs *rm, const CrcArgs *crc) {
  return lay.staged ? launch_route<TableRoute<true>>(g, args, lay, ar, stream, resident,
                                                     advance_out, rm, crc)
                    : launch_route<TableRoute<false>>(g, args, lay, ar, stream, resident,
                                                      advance_out, rm, crc);
}

int launch_layered_decode(const LayeredQcView &g, const DecodeArgs &args, const LayeredLayout &lay,
                          const LayeredArith &ar, void *stream, int *resident,
                          uint32_t *advance_out, const RmArgs *rm, const CrcArgs *crc) {
  return launch_route<CirculantRoute>(g, args, lay, ar, stream, resident, advance_out, rm, crc);
}

}  // namespace ldpc
