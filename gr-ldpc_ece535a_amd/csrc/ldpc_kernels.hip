// ldpc_kernels.hip -- belief-propagation decode kernels for gfx950 (MI355X).
//
// Hot path of ericdegroot/gr-ldpc_ece535a: the decode call inside
// ldpc_decoder_cb_impl::general_work (lib/ldpc_decoder_cb_impl.cc:155-164).
//
// Mapping ("small code" kernel, N <= 256, E <= 512, dc <= 8, dv <= 4):
//   * one 64-lane wave decodes one frame at a time; 4 independent waves per
//     256-thread workgroup, each with a private LDS slice; a wave leaves its
//     iteration loop on its own syndrome (per-frame early termination exactly
//     as the reference) and pulls the next frame from a launch-wide queue;
//   * lane l owns edges l, l+64, ... (S slots): its variable->check message
//     lives in VGPRs across iterations; the per-iteration exchange goes
//     through LDS (tanh values for the check pass, check->variable messages
//     for the column sums);
//   * every LDS gather is unconditional: unused neighbour entries point at a
//     per-wave dummy element holding the operation's identity (1.0 for the
//     tanh product, DBL_MAX for the min-sum minimum), or their contribution
//     is dropped with a select -- so a lane's loads issue back to back and the
//     wave waits once per phase instead of once per neighbour;
//   * lane l also owns columns l, l+64, ... for the hard decision; the hard
//     decision is a 64-bit wave ballot per 64 columns, the syndrome is
//     popcount(rowmask & hard) per row lane + one more ballot;
//   * per frame the only HBM traffic is its N input samples and its outputs.
// Arithmetic follows the reference operation for operation (same operand
// order, no contraction: built with -ffp-contract=off), in double
// (LDPC_PREC_F64) or float (LDPC_PREC_F32).
#include "ldpc_dispatch.hpp"
#include "ldpc_frame.hpp"

namespace ldpc {

// Persistent launch: `a.waves` waves; wave w decodes frame w, then frames
// a.waves + ticket++ until the batch is exhausted.  Frames stop after 1..cap
// iterations, so pulling work keeps every SIMD busy to the end instead of
// leaving it with a fixed share of the batch.
#ifdef LDPC_TIMELINE
// Diagnostic builds only (tools/timeline.py): per frame the 100 MHz realtime
// clock at its start and end and the wave's hardware ids.
constexpr int kTimelineFrames = 65536;
__device__ uint64_t g_timeline[4 * kTimelineFrames];
#endif

#ifndef LDPC_SMALL_MIN_BLOCKS
// occupancy hint: 3 waves per SIMD (for 4-wave workgroups the compiler's
// default, 1, gives the same register budget)
#define LDPC_SMALL_MIN_BLOCKS (kWavesPerBlock >= 4 ? 1 : 12 / kWavesPerBlock)
#endif
// MINB = LDPC_TP_MINB (four waves per SIMD, <= 128 VGPRs): the throughput build of the
// sum-product f64 kernel (several launches in flight share the CUs); one
// launch at a time runs faster with the larger register budget
// (profiles/round2/layout/ab_min_blocks.txt).
template <int PREC, int METHOD, int S, int NW, int DCN = kDcMax - 1, int DVN = kDvMax,
          int MINB = LDPC_SMALL_MIN_BLOCKS>
__global__ void __launch_bounds__(kThreads, MINB)
    decode_small_kernel(CodeView code, DecodeArgs a) {
  typedef typename Math<PREC>::Real Real;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int M = code.M;
  typedef Layout<Real, METHOD, S, NW, DVN> LW;
  constexpr SliceLayout L = LW::L;
  __shared__ typename Math<PREC>::Tab logtab[TabLds<PREC>::kN];
  if constexpr (METHOD == 1) stage_tab<PREC>(logtab);

  const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t c = a.claim;  // frames per claim (1 with static_stride)
  int64_t b = w * c;
  if (w >= a.waves || b >= a.B) return;
  int64_t bend = b + c;  // end of the wave's current claim

  // the wave's view of the code, in registers: wave_setup (ldpc_frame.hpp),
  // spelled out.  The call moves the VGPR / AGPR counts of three
  // instantiations of this kernel (profiles/round17/small_dispatch_isa.txt),
  // so the copy stays until that is settled; keep the two in step.
  WaveTables<S, NW> wt;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uint4 r = reinterpret_cast<const uint4 *>(code.erow)[lane + 64 * s];
    wt.rn[s][0] = r.x;
    wt.rn[s][1] = r.y;
    wt.rn[s][2] = r.z;
    wt.rn[s][3] = r.w;
    const uint2 c = reinterpret_cast<const uint2 *>(code.ecol)[lane + 64 * s];
    wt.cn[s][0] = c.x;
    wt.cn[s][1] = c.y;
  }
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const uint4 c = reinterpret_cast<const uint4 *>(code.cols)[lane + 64 * q];
    wt.ce[q][0] = c.x;
    wt.ce[q][1] = c.y;
    wt.cr[q][0] = c.z;
    wt.cr[q][1] = c.w;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int j = lane + 64 * q;
      wt.rowmask[q][k] = j < M ? code.rowmask[j * NW + k] : 0ull;
    }
  }

  Real *tb = reinterpret_cast<Real *>(smem + (size_t)wave * LW::per_wave) + L.tb;
  Real *eb = tb + (L.eb - L.tb);
  Real *rb = tb + (L.rb - L.tb);
  Real *sb = tb + (L.sb - L.tb);
  if constexpr (METHOD <= 1) {
    // ids -> LDS byte addresses of this wave's slice (see decode_frame).
    // Missing row neighbours -> the identity cell of the lane's 32-lane group,
    // missing column entries -> the lane's zero cell: banks no other lane of
    // the group reads (ldpc_layout.hpp)
    constexpr uint32_t R = sizeof(Real), kDummy = 64 * S;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const uint32_t cid = (uint32_t)field(wt.rn[s], 7);
      // padding cells (no edge) read zero cells, so their product T is 0, not 1
      relocate(wt.rn[s], DCN, lds_addr(tb), R,
               cid == kNone ? (uint32_t)(L.ebd - L.tb) + (lane & 31)
                            : kDummy + dpos_of(code, 2 * s + (lane >> 5)));
      const uint32_t ca = lds_addr(rb) / R + (cid == kNone ? (uint32_t)lane : cid);
      wt.rn[s][3] = (wt.rn[s][3] & 0xffffu) | (ca << 16);
      relocate(wt.cn[s], DVN - 1, lds_addr(eb), R, kDummy + (lane & 31));
    }
#pragma unroll
    for (int q = 0; q < NW; ++q) relocate(wt.ce[q], DVN, lds_addr(eb), R, kDummy + (lane & 31));
  }
  // column of each of the lane's positions, and the positions of the
  // columns of packed byte `lane` (8 bits each; N <= 256)
  int colq[NW];
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const uint32_t c = code.lane_col[lane + 64 * q];
    colq[q] = c == kNone ? -1 : (int)c;
  }
  uint32_t ppos[2] = {0u, 0u};
  if (lane < code.KB) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = M + 8 * lane + j;
      if (c < code.N) ppos[j >> 2] |= (uint32_t)code.col_lane[c] << (8 * (j & 3));
    }
  }

#ifndef LDPC_NO_PREFETCH
  // pull the samples of the frames the ticket queue hands out later into L2
  // (one frame per resident wave); the values are consumed by an empty asm
  // after the first frame, when the loads have long completed
  float pf[NW];
  {
    int64_t pb = (int64_t)a.waves * c + b;
    pb = pb < a.B ? pb : b;
    float ppol;
    const float *ps = frame_src(a, pb, ppol);
    (void)ppol;  // the prefetch only pulls the samples into L2
#pragma unroll
    for (int q = 0; q < NW; ++q) pf[q] = colq[q] >= 0 ? ps[(int64_t)colq[q] * a.elem_stride] : 0.0f;
  }
  bool first = true;
#endif
  while (b < a.B) {
#ifdef LDPC_TIMELINE
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    const uint64_t c_start = __builtin_amdgcn_s_memtime();
#endif
    const int64_t f = b;
    // the frame's channel samples, one load per lane and column position
    // (a permutation of the frame's N samples); positions past N are 0
    float xin[NW], pol;
    const float *src = frame_src(a, f, pol);
#pragma unroll
    for (int q = 0; q < NW; ++q)
      xin[q] = colq[q] >= 0 ? src[(int64_t)colq[q] * a.elem_stride] * pol : 0.0f;
    // decode_samples (ldpc_frame.hpp), spelled out: through the call this
    // kernel's frame prologue compiled to other instructions (same registers),
    // and the min-sum launch latencies at B = 16 and 256 measured 0.7-0.9 %
    // slower, outside the parent's spread (profiles/round17/small_dispatch_ab.txt,
    // job 1; with this copy they are back, job 2).  Keep the two in step.
    if constexpr (METHOD == 1) {
      bool bad = false;
#pragma unroll
      for (int q = 0; q < NW; ++q) bad |= !__builtin_isfinite(xin[q]);
      // the throughput build runs with fair_cycles 0 (batch_minb)
      constexpr bool kFair = MINB != LDPC_TP_MINB;
      if (__ballot(bad) == 0)
        decode_frame<PREC, METHOD, S, NW, DCN, DVN, true, Real, true, kFair>(
            code, a, f, wt, tb, eb, rb, sb, lane, logtab, xin, colq, ppos);
      else
        decode_frame<PREC, METHOD, S, NW, DCN, DVN, false, Real, true, kFair>(
            code, a, f, wt, tb, eb, rb, sb, lane, logtab, xin, colq, ppos);
    } else {
      decode_frame<PREC, METHOD, S, NW, DCN, DVN>(code, a, f, wt, tb, eb, rb, sb, lane, logtab,
                                                  xin, colq, ppos);
    }
#ifndef LDPC_NO_PREFETCH
    if (first) {
#pragma unroll
      for (int q = 0; q < NW; ++q) asm volatile("" ::"v"(pf[q]));
      first = false;
    }
#endif
#ifdef LDPC_TIMELINE
    if (lane == 0 && b < kTimelineFrames) {
      g_timeline[4 * b] = t_start;
      g_timeline[4 * b + 1] = __builtin_amdgcn_s_memrealtime();
      g_timeline[4 * b + 2] = (uint64_t)(uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |  // HW_ID
                              ((uint64_t)(uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);  // XCC_ID
      g_timeline[4 * b + 3] = __builtin_amdgcn_s_memtime() - c_start;  // core clocks
    }
#endif
    if (a.static_stride) {
      b += a.waves;
    } else if (++b == bend || b >= a.B) {
      // the claim is used up (or cut by the batch's end): the next one
      uint32_t t = 0;
      if (lane == 0) t = atomicAdd(a.ticket, (uint32_t)c) - a.ticket_base;
      b = (int64_t)a.waves * c + (int64_t)__builtin_amdgcn_readfirstlane((int)t);
      bend = b + c;
    }
  }
}

// ---------------------------------------------------------------------------
// Multi-wave kernel: one frame per S-wave workgroup, one edge per lane
// (mw_frame, ldpc_frame.hpp).
//
// At small batches the decode time is set by the frames that run to the
// iteration cap, i.e. by one frame's per-iteration latency.  Spreading a
// frame over S waves (on different SIMDs of the CU) divides the edge work of
// an iteration by S; the price is two workgroup barriers per iteration.
// ---------------------------------------------------------------------------

template <int PREC, int METHOD, int S, int NW>
__global__ void __launch_bounds__(64 * S) decode_mw_kernel(CodeView code, DecodeArgs a) {
  typedef typename Math<PREC>::Real Real;
  extern __shared__ __align__(16) unsigned char smem[];
  const MwLayout<Real, S, NW> L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = code.N;
  constexpr int kDummy = 64 * S;
  Real *tb = reinterpret_cast<Real *>(smem);
  Real *eb = reinterpret_cast<Real *>(smem + L.eb);
  Real *rb = reinterpret_cast<Real *>(smem + L.waves + (size_t)wave * L.per_wave);
  Real *sb = rb + 64 * NW;
  int *fslot = reinterpret_cast<int *>(smem + L.fslot);
  __shared__ typename Math<PREC>::Tab logtab[TabLds<PREC>::kN];
  if constexpr (METHOD == 1) stage_tab<PREC>(logtab);
  if (tid == 0) tb[kDummy] = METHOD == 1 ? Real(1) : Math<PREC>::max_();
  MwTables<NW> t;
  mw_setup<NW>(code, tid, t);

  int64_t b = blockIdx.x;
  while (b < a.B) {
    float pol;
    const float *src = frame_src(a, b, pol);
    uint64_t hard[NW];
    Real post[NW];
    int used = 0;
    const int weight = mw_frame<PREC, METHOD, S, NW>(code, a.max_iters, a.et_period, t, tb, eb,
                                                     rb, sb, logtab, src, pol, a.elem_stride,
                                                     hard, post, used);
    // outputs (wave 0)
    if (wave == 0) {
      if (lane == 0) {
        if (a.iters) a.iters[b] = used;
        if (a.synd) a.synd[b] = weight;
      }
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int c = t.colq[q];
        if (c >= 0) {
          if (a.bits) a.bits[b * N + c] = (uint8_t)((hard[q] >> lane) & 1);
          if (a.llr) a.llr[b * N + c] = (float)post[q];
        }
      }
      // (mw_packed_byte, spelled out: the call changes this kernel's register
      // counts in 75 instantiations, profiles/round17/small_dispatch_isa.txt)
      for (int p = lane; p < code.KB; p += 64) {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = code.M + 8 * p + j;
          if (c < N) {
            const int x = code.col_lane[c];  // position of column c
            o |= (uint32_t)((word_at<NW>(hard, x >> 6) >> (x & 63)) & 1) << (7 - j);
          }
        }
        a.packed[b * code.KB + p] = (uint8_t)o;
      }
    }
    wave_lds_sync();  // this wave's rb reads done before the next frame's writes
    if (a.static_stride) {
      __syncthreads();
      b += a.waves;
    } else {
      if (tid == 0) *fslot = (int)(atomicAdd(a.ticket, 1u) - a.ticket_base);
      __syncthreads();
      b = (int64_t)a.waves + (int64_t)*fslot;
    }
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
template <int PREC, int METHOD, int S, int NW, int DCN = kDcMax - 1, int DVN = kDvMax,
          int MINB = LDPC_SMALL_MIN_BLOCKS>
static int launch_one(const CodeView &code, const DecodeArgs &a, hipStream_t st) {
  typedef typename Math<PREC>::Real Real;
  const size_t lds = Layout<Real, METHOD, S, NW, DVN>::total;
  if (lds > 65536 &&
      hipFuncSetAttribute((const void *)decode_small_kernel<PREC, METHOD, S, NW, DCN, DVN, MINB>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -3;
  const dim3 grid((unsigned)((a.waves + kWavesPerBlock - 1) / kWavesPerBlock));
  hipLaunchKernelGGL((decode_small_kernel<PREC, METHOD, S, NW, DCN, DVN, MINB>), grid, dim3(kThreads),
                     lds, st, code, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int PREC, int METHOD, int S, int NW>
static int launch_mw(const CodeView &code, const DecodeArgs &a, hipStream_t st) {
  typedef typename Math<PREC>::Real Real;
  const size_t lds = MwLayout<Real, S, NW>().total;
  if (lds > 65536 &&
      hipFuncSetAttribute((const void *)decode_mw_kernel<PREC, METHOD, S, NW>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -3;
  hipLaunchKernelGGL((decode_mw_kernel<PREC, METHOD, S, NW>), dim3((unsigned)a.waves),
                     dim3(64 * S), lds, st, code, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

namespace {

// The batch launcher's policy over dispatch_small (ldpc_dispatch.hpp): every
// slot count; methods 2 and 3 (below, launch_decode) have one kernel per NW.
constexpr int kBatchSlotsMax = kSlotsMax;
// MINB of cell C.  Throughput mode (no issue-priority management: fair_cycles
// is 0) runs the 4-waves-per-SIMD build of the low-degree sum-product f64
// kernels at 3 and 4 slots.
template <class C>
constexpr int batch_minb(bool fair) {
  return C::LOW && (C::PREC == 0 || C::PREC == 3) && C::METHOD == 1 && (C::S == 3 || C::S == 4) &&
                 !fair
             ? LDPC_TP_MINB
             : LDPC_SMALL_MIN_BLOCKS;
}

struct LaunchOne {
  const CodeView &code;
  const DecodeArgs &a;
  hipStream_t st;
  template <class C>
  int operator()(C) const {
    constexpr int kTp = batch_minb<C>(false), kFairMinb = batch_minb<C>(true);
    if constexpr (kTp != kFairMinb)
      if (a.fair_cycles == 0)
        return launch_one<C::PREC, C::METHOD, C::S, C::NW, C::DCN, C::DVN, kTp>(code, a, st);
    return launch_one<C::PREC, C::METHOD, C::S, C::NW, C::DCN, C::DVN, kFairMinb>(code, a, st);
  }
};

// bit-flip (2) and hard decision (3): batch-only, one kernel per NW
template <int NW>
int launch_hard(const CodeView &code, const DecodeArgs &a, int method, hipStream_t st) {
  return method == 2 ? launch_one<1, 2, 1, NW>(code, a, st) : launch_one<1, 3, 1, NW>(code, a, st);
}

// the workgroup-per-frame kernel has the generic loops only
struct LaunchMw {
  const CodeView &code;
  const DecodeArgs &a;
  hipStream_t st;
  template <class C>
  int operator()(C) const {
    return launch_mw<C::PREC, C::METHOD, C::S, C::NW>(code, a, st);
  }
};

}  // namespace

int cu_count(int dev) {
  static std::atomic<int> cus[64];
  if (dev < 0 || dev >= 64) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (!n) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int resident_per_cu(std::atomic<int> &once, const void *fn, int threads, size_t lds, int cap) {
  int per_cu = once.load(std::memory_order_relaxed);
  if (!per_cu) {
    if (lds > 65536 &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return 0;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) != hipSuccess || n < 1)
      n = 1;
    per_cu = std::min(n, cap);
    once.store(per_cu, std::memory_order_relaxed);
  }
  return per_cu;
}

bool resident_workgroups(const void *fn, int threads, int lds, int lds_limit, int &cache) {
  if (cache != 0) return true;
  int per_cu = 0, dev = 0;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, (size_t)lds) != hipSuccess ||
      per_cu < 1 || hipGetDevice(&dev) != hipSuccess)
    return false;
  cache = per_cu * cu_count(dev);
  return true;
}

bool wg_launch(const void *fn, int threads, int lds, int &cache, DecodeArgs &a,
               uint32_t *advance_out) {
  if (!resident_workgroups(fn, threads, lds, kWgLdsLimit, cache)) return false;
  a.waves = (int)std::min<int64_t>(a.B, cache);
  *advance_out = a.static_stride ? 0u : (uint32_t)a.B;
  return true;
}

int launch_decode(const CodeView &code, const DecodeArgs &args, int method, int prec, int slots,
                  int nw, int waves_per_cu, int schedule, void *stream, uint32_t *advance_out) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  *advance_out = 0;
  if (args.B <= 0) return 0;
  DecodeArgs a = args;
  // CUs of the current device
  int dev = 0;
  const int cus = hipGetDevice(&dev) == hipSuccess ? cu_count(dev) : 256;
#ifndef LDPC_SMALL_WPC
#define LDPC_SMALL_WPC 12
#endif
  if (waves_per_cu <= 0) waves_per_cu = LDPC_SMALL_WPC;
  // schedule: 1 one wave per frame, 2 one workgroup of `slots` waves per
  // frame, 0 auto.  Measured (bench.py --sweep-batch): with round 2's compact
  // arithmetic the one-wave form was as fast as the workgroup form for every
  // method at B = 16..256 and faster from B = 1024 on
  // (profiles/round1/schedules_sweep.txt); with the exact sum-product
  // arithmetic (precision 0 / 2) a frame's iteration is long enough that
  // splitting it over `slots` waves lowers the latency of small launches --
  // 50 iterations of one frame 60.8 vs 88.6 us, B = 256 0.066 vs 0.097 ms --
  // while the one-wave form stays ahead at B = 1024 (0.0995 vs 0.113 ms;
  // profiles/round3/latency_schedules_exact.txt).  Auto therefore takes the
  // workgroup form for exact sum-product launches of <= kMwAutoMax frames
  // (the block's dependent window launches) and the one-wave form otherwise.
  constexpr int kMwAutoMax = 512;
  const bool mw = schedule == 2 || (schedule == 0 && method == 1 && (prec == 0 || prec == 2) &&
                                    a.B <= kMwAutoMax);
  if (mw) {
    const int64_t frames_in_flight = std::max<int64_t>(1, (int64_t)waves_per_cu * cus / slots);
    a.waves = (int)std::min<int64_t>((int64_t)a.B, frames_in_flight);
  } else {
    const int64_t w = std::min<int64_t>((int64_t)a.B, (int64_t)waves_per_cu * cus);
    a.waves = (int)((w + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock);
  }
  // the one-wave kernel's fast modes claim several frames per queue add when
  // the batch is several times the resident waves (one counter word serves
  // ~88 adds per us: ring_claim, ldpc_kernels.hpp); smaller batches, the
  // workgroup form and fixed strides take one (every wave's first claim
  // starts at once: claims of several frames would serialise a small batch)
  const int64_t waves_max = (int64_t)waves_per_cu * cus;
  a.claim = mw || a.static_stride || a.B < 4 * waves_max ? 1 : ring_claim(method, prec);
  int rc = -2;
  if (mw && method <= 1)
    rc = dispatch_small<kBatchSlotsMax>(method, prec, slots, nw, kernel_shape(nw, slots, kDcMax, kDvMax),
                                        LaunchMw{code, a, st});
  else if (method == 2 || method == 3)
    rc = nw == 1 ? launch_hard<1>(code, a, method, st) : nw == 4 ? launch_hard<4>(code, a, method, st) : -2;
  else
    rc = dispatch_small<kBatchSlotsMax>(method, prec, slots, nw,
                                        kernel_shape(nw, slots, code.dc_max, code.dv_max),
                                        LaunchOne{code, a, st});
  if (rc == 0 && !a.static_stride)
    *advance_out = (uint32_t)(a.claim * ((a.B + a.claim - 1) / a.claim));
  return rc;
}

}  // namespace ldpc

#ifdef LDPC_TIMELINE
extern "C" int ldpc_debug_timeline(uint64_t *host, int frames) {
  if (frames > ldpc::kTimelineFrames) frames = ldpc::kTimelineFrames;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(ldpc::g_timeline), sizeof(uint64_t) * 4 * frames) ==
                 hipSuccess
             ? frames
             : -1;
}
#endif
