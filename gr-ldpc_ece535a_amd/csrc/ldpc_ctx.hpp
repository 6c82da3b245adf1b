// ldpc_ctx.hpp -- the context behind include/ldpc_hip.h, private to the C ABI's
// files (ldpc_capi_*.hip), and the helpers that cross them.
//
// struct ldpc_ctx is one value member per owner.  A group that owns device
// memory, pinned memory, streams or events has one release(), which frees what
// the group owns and nulls the pointers; ldpc_destroy is the ordered sequence
// of those calls.  No destructor frees device state: the frees are ordered
// against the synchronisations in ldpc_destroy, which also runs on a
// half-built context.  Nothing declared here is exported from the library.
#pragma once

#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "ldpc_capi_host.hpp"
#include "ldpc_crc.hpp"
#include "ldpc_graph.hpp"
#include "ldpc_kernels.hpp"
#include "ldpc_layered.hpp"
#include "ldpc_onchip.hpp"
#include "ldpc_rate_match.hpp"

#pragma GCC visibility push(hidden)

namespace ldpc {
namespace capi {

// Small-code frame queues: counters per context, one per 256 bytes so that
// the streams' queues never share a cache line (atomics on one line
// serialise in its L2 channel).
constexpr int kTicketSlots = 64;
constexpr int kTicketStride = 64;  // in uint32_t

template <typename T>
inline void free_device(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

template <typename T>
inline void free_pinned(T *&p) {
  if (p) (void)hipHostFree(p);
  p = nullptr;
}

// Host threads that gather a span's samples into pinned memory (copy_span):
// the block's spans are gr_complex, and taking the real parts of 4096 frames
// (2 MB read) on one thread is ~100-180 us in front of the call's first round.
// Pieces are handed out by an atomic counter; the calling thread gathers too
// and sends each piece to the device, in order, once it is ready.
struct GatherPool {
  static constexpr int kThreads = 3;      // helpers (plus the calling thread)
  static constexpr int64_t kPiece = 1 << 14;  // samples per piece gathered
  // samples per copy to the device: a copy costs ~8 us of its own (64 KB
  // copies, one per gathered piece, took 16 x 15.6 us for a 1 MB span,
  // profiles/round5/block_trace.txt)
  static constexpr int64_t kCopy = 1 << 18;
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t gen = 0;
  bool quit = false;
  const float *in = nullptr;
  float *h = nullptr;
  int64_t S = 0, npieces = 0;
  int stride = 1;
  std::atomic<int64_t> next{0};
  std::unique_ptr<std::atomic<uint64_t>[]> ready;
  int64_t ready_cap = 0;
  void gather(int64_t p) const {
    const int64_t i0 = p * kPiece, i1 = std::min(S, i0 + kPiece);
    if (stride == 1)
      memcpy(h + i0, in + i0, (size_t)(i1 - i0) * 4);
    else if (stride == 2)  // gr_complex real parts: a constant stride vectorises
      for (int64_t i = i0; i < i1; ++i) h[i] = in[2 * i];
    else
      for (int64_t i = i0; i < i1; ++i) h[i] = in[i * stride];
  }
  void worker() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return quit || gen != seen; });
        if (quit) return;
        seen = gen;
      }
      for (;;) {
        const int64_t p = next.fetch_add(1);
        if (p >= npieces) break;
        gather(p);
        ready[p].store(seen, std::memory_order_release);
      }
    }
  }
  ~GatherPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
};

}  // namespace capi
}  // namespace ldpc

struct ldpc_ctx {
  // shape, and the decoder's H on the host (ldpc_capi_create.hip)
  struct Code {
    int M = 0, N = 0, E = 0, K = 0, KB = 0, dc_max = 0, dv_max = 0, dc_min = 0;
    std::vector<uint8_t> H;         // the decoder's (reordered) H; empty beyond the small-code limits
    std::vector<int32_t> rp, ci;    // host CSR of the decoder's H
    // a quasi-cyclic context (ldpc_create_qc) remembers its base matrix
    int qc_mb = 0, qc_nb = 0, qc_Z = 0;  // qc_Z == 0: not a QC context
    std::vector<int32_t> qc_shifts;
  } code;

  // small-code path (ldpc_kernels.hip): the device tables of build_tables
  // and the launch knobs (ldpc_capi_create.hip)
  struct Small {
    ldpc::EdgeRowRec *d_erow = nullptr;
    ldpc::EdgeColRec *d_ecol = nullptr;
    ldpc::ColRec *d_cols = nullptr;
    uint64_t *d_rowmask = nullptr;
    uint16_t *d_lane_col = nullptr;  // small-code LDS layout (ldpc_layout.hpp)
    uint8_t *d_col_lane = nullptr;
    uint64_t dpos[2] = {0, 0};
    int layout_model[5] = {0, 0, 0, 0, 0};  // searched?, modelled cc / ec, plain cc / ec
    int waves_per_cu = 0;           // 0: kernel default
    // launch mode (ldpc_set_launch_mode): issue-priority threshold of the
    // small-code kernel, core clocks (profiles/round1/ab_fair_threshold_warm.txt:
    // 1800 is the best of 1200..3000 for one launch at a time); 0 = off
    uint32_t fair_cycles = 1800;
    int schedule = 0;               // 0 auto, 1 wave per frame, 2 workgroup per frame
    void release();
  } small;

  // large-code path (ldpc_graph.hip): H as CSR + CSC, messages in a workspace
  // (tables: ldpc_capi_create.hip; workspace and stream order: ldpc_capi_decode.hip)
  struct Graph {
    bool on = false;
    int32_t *d_rp = nullptr, *d_ci = nullptr, *d_cp = nullptr, *d_ce = nullptr, *d_cr = nullptr;
    void *d_work = nullptr;
    size_t work_bytes = 0;
    size_t work_limit = (size_t)8 << 30;
    // the workspace is shared, so launches on a different stream than the
    // previous one first wait for it (done)
    void *stream = nullptr;
    hipEvent_t done = nullptr;
    // large-code min-sum runs on the narrow-chunk pipeline (ldpc_graph_msn.hip)
    bool narrow = false;  // large code with the min-sum pipeline's tables (M <= kMsnMaxRows)
    ldpc::MsnTables msn;  // storage order of the narrow pipeline
    int32_t *d_msn[4] = {nullptr, nullptr, nullptr, nullptr};  // rx cx corig cpos
    ldpc::MsnDesc *d_msnd[2] = {nullptr, nullptr};             // rdesc cdesc
    int32_t *h_ctrl = nullptr;  // pinned progress words of the min-sum pipeline
    void release();  // synchronises the device before the workspace goes
  } graph;

  // on-chip path (ldpc_onchip.hip, LDPC_FLAG_ONCHIP): a large-code context
  // whose min-sum / sum-product decodes run one frame per workgroup in LDS,
  // with frame queues (queues.d_tickets) like the small-code path's
  struct Onchip {
    bool on = false;
    uint32_t *d_erow = nullptr, *d_ecol = nullptr, *d_rows = nullptr, *d_cols = nullptr;
    uint16_t *d_ci = nullptr, *d_ce = nullptr;
    int resident[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // workgroups the device holds, per kernel
    void release();
  } onchip;

  // layered min-sum (ldpc_layered.hip, ldpc_decode_layered*; ldpc_capi_layered.hip),
  // on any context whose code fits: the plan in force (made on first use, or
  // the caller's), and the tables built and uploaded from it by the first
  // decode after it changed
  struct Layered {
    std::vector<int32_t> of_row;
    int L = 0;            // 0: no plan yet
    bool ready = false;   // f64 / f32 are those of of_row, and the code fits float
    bool tabs = false;    // the device tables are those of of_row (float and q8 decodes share them)
    ldpc::LayeredLayout f64{}, f32{};
    uint32_t *d_rows = nullptr, *d_off = nullptr;
    uint16_t *d_ci = nullptr, *d_order = nullptr;
    int resident[2] = {0, 0};  // workgroups the device holds, f64 / f32 kernel
    // on a quasi-cyclic context the planner's plan is the block rows, and
    // while that plan is in force (and LDPC_FLAG_QC_TABLES is not set) layered
    // decodes run the circulant kernel (ldpc_layered.hip CirculantRoute) from
    // the base tables d_qc_*
    bool qc_tables = false;   // LDPC_FLAG_QC_TABLES
    bool qc = false;          // the tables uploaded are the circulant kernel's
    uint32_t *d_qc_rows = nullptr, *d_qc_ent = nullptr;
    int qc_rows = 0;          // block rows in d_qc_rows (those with an entry)
    // fixed-point layered min-sum (ldpc_layered.hip Q8Arith, ldpc_decode_layered_q8*):
    // the same plan and device tables, a layout and limits of its own
    bool q8_ready = false;    // q8 is that of of_row, and the code fits
    ldpc::LayeredLayout q8{};
    int q8_resident = 0;      // workgroups the device holds of the kernel q8 selects
    // the same of the kernels whose frame load recovers rate-matched samples
    // (ldpc_decode_layered*_rm*): f64 / f32, q8
    int rm_resident[2] = {0, 0}, rm_q8_resident = 0;
    void release();  // the device tables (also when a new plan replaces them)
  } layered;

  // rate matching (ldpc_set_rate_match; ldpc_rate_match.hpp): the context's
  // pattern, checked when it was set.  The default is the identity.
  struct RateMatch {
    int punct = 0, filler = 0, ncb = 0;
  } rm;

  // the code-block CRC (ldpc_set_crc; ldpc_crc.hpp; ldpc_capi_layered.hip):
  // len == 0 is off.  The weights of the A block positions on the device (d_w,
  // those of (w_len, poly, A): they outlive an off, so that turning the same
  // CRC on again is host work), rebuilt when another CRC or another filler
  // count is set; the remainders
  // of the last layered decode (d_rem, grown with B), its frames and stream;
  // and the workgroups the device holds of the layered kernels that check it
  // ([rate-matched][arithmetic]).
  struct Crc {
    int len = 0, mode = 0, A = 0, w_len = 0;
    uint32_t poly = 0;
    uint32_t *d_w = nullptr, *d_rem = nullptr;
    int rem_cap = 0, last_B = 0;
    void *last_stream = nullptr;
    int resident[2][3] = {{0, 0, 0}, {0, 0, 0}};
    void release();
  } crc;

  // device encoder (built on first ldpc_encode_device; ldpc_capi_encode.hip):
  // kind 1 small (A = H_p^-1 H_d bit rows in d_A), 2 IRA staircase, 3
  // quasi-cyclic with a dual-diagonal parity part (the step program of
  // ldpc_qc_enc.hpp in d_qc), -1 no systematic encoder
  struct Encoder {
    int kind = 0;
    uint64_t *d_A = nullptr;
    uint32_t *d_qc = nullptr;
    int qc_threads = 0, qc_lds = 0;
    bool qc_lds_allowed = false;
    std::string err;
    void release();
  } encoder;

  // staging of host-buffer decodes and of window decodes (ldpc_capi_decode.hip)
  struct Stage {
    void *d = nullptr;
    size_t d_bytes = 0;
    float *h = nullptr;  // pinned host staging of host-buffer decodes
    size_t h_bytes = 0;
    bool h_busy = false;  // a copy out of h may still be running (ldpc_stage_span)
    std::unique_ptr<ldpc::capi::GatherPool> gather;  // copy_span's helpers (made on first use)
    // ldpc_decode_windows: the staged sample span (device), window list and
    // frames; span_samples > 0 while the staged span may be reused
    void *d_span = nullptr;
    size_t span_bytes = 0;
    int64_t *h_win = nullptr;
    size_t h_win_bytes = 0;
    int64_t span_samples = 0;
    // LDPC_BLOCK_PROFILE=1: also the host time split of ldpc_decode_windows,
    // printed by ldpc_destroy (span staging, window list + launch, wait, result
    // copy); =2 also a line per call
    bool profile = getenv("LDPC_BLOCK_PROFILE") != nullptr;
    bool trace = profile && getenv("LDPC_BLOCK_PROFILE")[0] == '2';  // a line per call
    double prof[5] = {0, 0, 0, 0, 0};
    long long calls = 0, windows = 0;
    void release();
  } stage;

  // the window server (ldpc_serve.hip, ldpc_serve_*; ldpc_capi_serve.hip):
  // mapped pinned memory [round word | keys | result granules] for cap
  // windows, the device copy of the round word, and the running launch's
  // parameters
  struct Serve {
    bool serving = false;
    uint8_t *h = nullptr;
    int64_t cap = 0;
    uint64_t *d_ctl = nullptr;
    int64_t *d_keys = nullptr;  // the round's keys as the poller copies them
    uint32_t epoch = 0;  // the last round posted (grows across launches)
    int method = 0, iters = 0, prec = 0;
    int launches = 0, rounds = 0;
    int workgroups = 0;  // decoder workgroups of the running launch
    // LDPC_SERVE_DEBUG: rounds, host us, poller's sight -> publication, ->
    // last key read, -> last result stored (us)
    double dbg[6] = {0, 0, 0, 0, 0, 0};  // ... and the host's sight of the first result
    bool debug = false;  // LDPC_SERVE_DEBUG, read when a launch starts
    bool test_skip_check = false;  // ldpc_test_hook(LDPC_TEST_SERVE_UNCHECKED)
    void release();
  } serve;

  // the frame ring (ldpc_ring_*, ldpc_ring.hip; ldpc_capi_ring.hip): mapped
  // host memory [kRingSlots descriptors | kRingSlots completion words], device
  // memory [per-slot frame counters | queue head], the launch's own stream and
  // an event recorded behind the launch (complete = the launch has ended)
  struct Ring {
    bool on = false;  // a session is open (ldpc_ring_begin .. ldpc_ring_end)
    int method = 0, iters = 0, et = 1, prec = 0;
    uint8_t *h = nullptr;
    uint32_t *d = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr, user_ev = nullptr;
    void *user_stream = nullptr;
    uint64_t next = 0;      // the next batch's sequence number (grows across sessions)
    int64_t frames = 0;     // tickets posted so far (the next batch's start)
    uint64_t first = 0;     // the session's first batch
    int64_t first_frame = 0;
    int64_t start[ldpc::kRingSlots] = {};  // start ticket of the batch in each slot
    int launches = 0, workgroups = 0;
    bool clean = false;  // d zeroed for the next launch already
    void release();  // synchronises the ring's stream before it is destroyed
  } ring;

  // frame queues and streams (ldpc_capi_queues.hip)
  struct Queues {
    // small-code frame queues: one monotonic counter per stream that has
    // launched on this context (ldpc_kernels.hpp DecodeArgs::ticket)
    uint32_t *d_tickets = nullptr;
    struct Queue {
      void *stream;
      uint32_t base;  // counter value at the start of the next launch
    };
    std::vector<Queue> list;
    // in-flight stream set for throughput callers (ldpc_ctx_streams): streams
    // verified to run concurrently, i.e. on distinct hardware queues
    std::vector<hipStream_t> tp_streams;
    uint32_t *d_probe = nullptr;
    void release();  // synchronises each stream of the set before it is destroyed
  } queues;

  // what the whole context shares: the small-code kernels' shape of the code
  // (edge slots per lane, 64-bit words per frame, row slots; set by
  // build_tables, read by the decode, server and ring launches), the device,
  // the context's stream and its last error
  int slots = 0, nw = 0, rs = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
};

namespace ldpc {
namespace capi {

// ---- ldpc_capi_create.hip ----
int set_err(ldpc_ctx *ctx, int code, const std::string &msg);  // ctx NULL: the create error
int hip_err(ldpc_ctx *ctx, hipError_t e, const char *what);

// One table to the device; a chain of uploads stops at the first failure
// (failed names it, e is its error).
template <typename T>
bool upload(T **dst, const std::vector<T> &src, const char *what, const char *&failed,
            hipError_t &e) {
  if (failed) return false;
  if ((e = hipMalloc((void **)dst, std::max<size_t>(src.size(), 1) * sizeof(T))) != hipSuccess ||
      (!src.empty() &&
       (e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice)) !=
           hipSuccess)) {
    failed = what;
    return false;
  }
  return true;
}

// ---- ldpc_capi_serve.hip ----
// Ends a running window server: posts its quit round and waits for the
// launch to finish, so whatever the caller enqueues next does not queue
// behind a launch that polls for rounds.
void serve_stop_running(ldpc_ctx *ctx);
inline void serve_stop(ldpc_ctx *ctx) {
  if (ctx && ctx->serve.serving) serve_stop_running(ctx);
}

// ---- ldpc_capi_queues.hip ----
// The zeroed counter array, uploaded once per context (upload's conventions).
bool ensure_tickets(ldpc_ctx *ctx, const char *&failed, hipError_t &e);
// The frame-queue counter of stream `st` on this context: q is its slot in
// ctx->queues.list / ctx->queues.d_tickets.
int stream_queue(ldpc_ctx *ctx, void *st, size_t &q);
// Binds a launch to stream `st`'s queue: a.ticket, ticket_base, static_stride
// (a fixed stride for iteration caps <= 10) and waves = 0; q as stream_queue's.
int bind_queue(ldpc_ctx *ctx, void *st, int max_iters, ldpc::DecodeArgs &a, size_t &q);
// After the launch was enqueued: `advance` is what it adds to the counter
// (the launcher's *advance_out; 0 with a fixed stride).
void commit_queue(ldpc_ctx *ctx, size_t q, uint32_t advance);

// ---- ldpc_capi_decode.hip ----
int check_decode_args(ldpc_ctx *ctx, int &method, int max_iters, int et_period, int precision,
                      int B, int elem_stride, int64_t cw_stride);
ldpc::CodeView code_view(const ldpc_ctx *ctx);
// The launch arguments every decode starts from (no queue, no polarity pair).
ldpc::DecodeArgs make_args(const float *d_in, int64_t cw_stride, int elem_stride, float polarity,
                           int B, int max_iters, int et_period, uint8_t *d_packed, uint8_t *d_bits,
                           int32_t *d_iters, int32_t *d_synd, float *d_llr,
                           const int64_t *d_win = nullptr);
// Enqueues one decode of device-resident frames.  pm_half > 0: B = 2 pm_half
// and frames pm_half.. re-decode windows 0..pm_half-1 with -polarity
// (DecodeArgs::pm_half), in the same launch on the small-code path.
int decode_device_impl(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                       const float *d_in, int64_t cw_stride, int elem_stride, float polarity,
                       int B, int pm_half, uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                       int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                       float *d_llr_out_opt, void *hip_stream, const int64_t *d_win = nullptr);
// Host-buffer decode (synchronous), staged through the pinned buffer; both:
// the outputs are 2B frames, both polarities.  layered: the decode is a
// layered one in that arithmetic (method unused).  rm (layered only): a frame is
// rm_total rate-matched samples at cw_stride, elem_stride 1.
int decode_host_impl(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                     const float *in, int64_t n_in_floats, int64_t cw_stride, int elem_stride,
                     float polarity, int B, bool both, uint8_t *out_packed, uint8_t *out_bits_opt,
                     int32_t *iters_used_opt, int32_t *syn_weight_opt, float *llr_out_opt,
                     const ldpc::LayeredArith *layered = nullptr,
                     const ldpc::RmArgs *rm = nullptr, int64_t rm_total = 0);

// ---- ldpc_capi_layered.hip ----
// What a layered decode needs beyond check_decode_args (no ring session, the
// arithmetic's parameters, tables for the plan in force, a frame that fits).
int layered_arith_ready(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int precision);
// decode_device_impl for the layered kernel in the arithmetic `ar`.
// rm: the frames are rate-matched samples, recovered by the frame load
// (cw_stride is then rx_stride, elem_stride 1).
int layered_device_impl(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int max_iters, int et_period,
                        int precision, const float *d_in, int64_t cw_stride, int elem_stride,
                        float polarity, int B, uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                        int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                        float *d_llr_out_opt, void *hip_stream,
                        const ldpc::RmArgs *rm = nullptr);
// Checks (len, poly) and the block A = K - filler > len, then builds and
// uploads the A weights and makes them the context's CRC (its mode stays).
// LDPC_EINVAL with the offending value, and nothing changed, otherwise.
int crc_upload(ldpc_ctx *ctx, int len, uint32_t poly, int filler);
// Room for B remainders in the context's result array.
int crc_results_room(ldpc_ctx *ctx, int B);

// ---- ldpc_capi_encode.hip ----
// The context's pattern and a call's transmissions, resolved into rm; *total:
// the samples per frame.  LDPC_EINVAL with the offending value otherwise.
int rate_match_args(ldpc_ctx *ctx, int n_tx, const int32_t *k0, const int32_t *e,
                    float unreceived_lci, ldpc::RmArgs &rm, int64_t *total);

}  // namespace capi
}  // namespace ldpc

#pragma GCC visibility pop
