// ldpc_capi_ring.hip -- the C ABI of include/ldpc_hip.h: the host side of the
// frame ring (ldpc_ring.hip, ldpc_ring_*).  One persistent launch takes
// batches of device-resident frames from descriptors in mapped host memory.
// Owns the context's ring group (ldpc_ctx.hpp).
#include <chrono>

#include "ldpc_ctx.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Ring::release() {
  if (stream) {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }
  if (ev) (void)hipEventDestroy(ev);
  if (user_ev) (void)hipEventDestroy(user_ev);
  stream = nullptr;
  ev = user_ev = nullptr;
  free_pinned(h);
  free_device(d);
}

namespace {

// Mapped host memory: kRingSlots 64-byte descriptors, then kRingSlots
// completion words.  Device memory: kRingSlots frame counters, one 256-byte
// line each, then the queue head on a line of its own.
constexpr size_t kRingCompOff = sizeof(ldpc::RingDesc) * ldpc::kRingSlots;
constexpr size_t kRingHostBytes = kRingCompOff + 8 * ldpc::kRingSlots;
constexpr size_t kRingTicketOff = (size_t)ldpc::kRingSlots * ldpc::kRingDoneStride;  // in u32
constexpr size_t kRingMirrorOff = 4 * (kRingTicketOff + 64);  // bytes: the descriptor mirror
constexpr size_t kRingLockOff =
    kRingMirrorOff + sizeof(ldpc::RingDesc) * ldpc::kRingSlots * ldpc::kRingXcds;
constexpr size_t kRingDevBytes = kRingLockOff + 8 * ldpc::kRingSlots * ldpc::kRingXcds;
constexpr uint64_t kRingDeadlineTicks = 5000000;  // 50 ms without a batch: a wave leaves
constexpr double kRingTimeoutS = 10.0;

bool ring_done(ldpc_ctx *ctx, uint64_t q) {
  return __atomic_load_n(reinterpret_cast<uint64_t *>(ctx->ring.h + kRingCompOff) +
                             q % ldpc::kRingSlots,
                         __ATOMIC_ACQUIRE) >= q + 1;
}

// Writes batch q's descriptor: words 1..7 tagged with (q + 1) mod 2^16 in bits
// 48..63, then word 0 = q + 1 (x86 stores are ordered; the device accepts the
// line only when all eight agree, ldpc_ring.hip locate).
void ring_write_desc(ldpc_ctx *ctx, uint64_t q, int64_t start, const void *in, int64_t cw,
                     void *packed, void *iters, void *synd, int B, int quit) {
  uint64_t *w = reinterpret_cast<uint64_t *>(ctx->ring.h) + 8 * (q % ldpc::kRingSlots);
  const uint64_t tag = ((q + 1) & 0xFFFFu) << 48, pay = (1ull << 48) - 1;
  const uint64_t v[7] = {(uint64_t)start, (uint64_t)(uintptr_t)in, (uint64_t)cw,
                         (uint64_t)(uintptr_t)packed, (uint64_t)(uintptr_t)iters,
                         (uint64_t)(uintptr_t)synd,
                         (uint64_t)(uint32_t)B | ((uint64_t)(quit ? 1 : 0) << 32)};
  for (int j = 0; j < 7; ++j) __atomic_store_n(w + 1 + j, (v[j] & pay) | tag, __ATOMIC_RELAXED);
  __atomic_store_n(w, q + 1, __ATOMIC_RELEASE);
}

// Launches the ring from batch `cursor` (every earlier batch complete), its
// first ticket `ticket0`: counters and queue head zeroed first, on the ring's
// stream, and the event recorded behind the launch.
int ring_launch(ldpc_ctx *ctx, uint64_t cursor, int64_t ticket0) {
  ldpc_ctx::Ring &rg = ctx->ring;
  hipError_t e;
  if ((e = hipSetDevice(ctx->device)) != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  // (zeroed behind the previous session's launch by ldpc_ring_end, off the
  // next session's critical path; a relaunch zeroes here)
  if (!rg.clean && (e = hipMemsetAsync(rg.d, 0, kRingDevBytes, rg.stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemsetAsync(ring)");
  rg.clean = false;
  void *dh = nullptr;
  if ((e = hipHostGetDevicePointer(&dh, rg.h, 0)) != hipSuccess)
    return hip_err(ctx, e, "hipHostGetDevicePointer(ring)");
  ldpc::RingArgs r{};
  r.desc = reinterpret_cast<const ldpc::RingDesc *>(dh);
  r.comp = reinterpret_cast<uint64_t *>((uint8_t *)dh + kRingCompOff);
  r.done = rg.d;
  r.ticket = rg.d + kRingTicketOff;
  r.mirror = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(rg.d) + kRingMirrorOff);
  r.lock = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(rg.d) + kRingLockOff);
  r.ticket0 = ticket0;
  r.cursor0 = cursor;
  r.deadline = kRingDeadlineTicks;
  r.max_iters = rg.iters;
  r.et_period = rg.et;
  int wg = 0;
  const int rc = ldpc::launch_ring(code_view(ctx), r, rg.method, rg.prec, ctx->slots, ctx->nw,
                                   ctx->device, rg.stream, &wg);
  if (rc == -2) return set_err(ctx, LDPC_EUNSUPPORTED, "no frame ring for this code shape");
  if (rc != 0) return hip_err(ctx, hipGetLastError(), "frame ring launch");
  rg.workgroups = wg;
  rg.launches += 1;
  if ((e = hipEventRecord(rg.ev, rg.stream)) != hipSuccess)
    return hip_err(ctx, e, "hipEventRecord(ring)");
  return LDPC_OK;
}

// A launch whose waves all left on the deadline (no batch for 50 ms) has
// ended: if posted batches are not complete, launch again from the first of
// them.  Its frames are decoded again from frame 0 -- a wave may have left
// holding a ticket of a batch it never saw -- and the frame counters start
// at zero, so a batch completes exactly once.
// `upto`: batches before it are the ones that must complete (a posted quit
// descriptor is not one of them).
int ring_revive(ldpc_ctx *ctx, uint64_t upto) {
  const hipError_t q = hipEventQuery(ctx->ring.ev);
  if (q == hipErrorNotReady) return LDPC_OK;
  if (q != hipSuccess) return hip_err(ctx, q, "frame ring");
  uint64_t first = upto;
  const uint64_t lo = std::max<uint64_t>(
      ctx->ring.first, upto > (uint64_t)ldpc::kRingSlots ? upto - ldpc::kRingSlots : 0);
  for (uint64_t b = lo; b < upto; ++b)
    if (!ring_done(ctx, b)) {
      first = b;
      break;
    }
  if (first == upto) return LDPC_OK;  // nothing outstanding: relaunch on the next post
  return ring_launch(ctx, first, ctx->ring.start[first % ldpc::kRingSlots]);
}

// Waits until batch q is complete (q < ring.next).
int ring_wait_impl(ldpc_ctx *ctx, uint64_t q) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 1; !ring_done(ctx, q); ++spins) {
    if ((spins & 0x3FFu) == 0) {
      const int rc = ring_revive(ctx, q + 1);
      if (rc != LDPC_OK) return rc;
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >
          kRingTimeoutS)
        return set_err(ctx, LDPC_ETIMEOUT, "a frame ring batch passed its timeout");
    }
  }
  return LDPC_OK;
}

// Posts one descriptor (a batch, or quit): waits for its slot's previous
// batch, writes the line, and relaunches a launch that has ended.
int64_t ring_post_impl(ldpc_ctx *ctx, const float *d_in, int64_t cw, int B, uint8_t *packed,
                       int32_t *iters, int32_t *synd, int quit) {
  ldpc_ctx::Ring &rg = ctx->ring;
  const uint64_t q = rg.next;
  if (q >= rg.first + ldpc::kRingSlots) {
    const int rc = ring_wait_impl(ctx, q - ldpc::kRingSlots);
    if (rc != LDPC_OK) return rc;
  }
  rg.start[q % ldpc::kRingSlots] = rg.frames;
  ring_write_desc(ctx, q, rg.frames, d_in, cw, packed, iters, synd, B, quit);
  rg.next = q + 1;
  rg.frames += B;
  // a launch that has ended meanwhile would never see it
  // (a quit descriptor alone needs no launch: nothing would be decoded)
  const int rc = ring_revive(ctx, quit ? q : q + 1);
  return rc != LDPC_OK ? rc : (int64_t)q;
}

}  // namespace

extern "C" {

int ldpc_ring_begin(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                    void *hip_stream) {
  if (!ctx) return LDPC_EINVAL;
  ldpc_ctx::Ring &rg = ctx->ring;
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, 1, 1, ctx->code.N);
  if (rc != LDPC_OK) return rc;
  if (rg.on) return set_err(ctx, LDPC_EINVAL, "a frame ring session is open (ldpc_ring_end)");
  if (ctx->onchip.on)
    return set_err(ctx, LDPC_EUNSUPPORTED,
                   "the frame ring does not run on an on-chip context (small-code kernels only); "
                   "use ldpc_decode_device");
  if (ctx->graph.on || (method != 0 && method != 1))
    return set_err(ctx, LDPC_EUNSUPPORTED,
                   "the frame ring takes min-sum / sum-product on small codes");
  serve_stop(ctx);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  if (!rg.h && (e = hipHostMalloc((void **)&rg.h, kRingHostBytes,
                                  hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
    return hip_err(ctx, e, "hipHostMalloc(ring)");
  if (!rg.d && (e = hipMalloc((void **)&rg.d, kRingDevBytes)) != hipSuccess)
    return hip_err(ctx, e, "hipMalloc(ring)");
  if (!rg.stream && (e = hipStreamCreateWithFlags(&rg.stream, hipStreamNonBlocking)) != hipSuccess)
    return hip_err(ctx, e, "hipStreamCreate(ring)");
  if (!rg.ev && (e = hipEventCreateWithFlags(&rg.ev, hipEventDisableTiming)) != hipSuccess)
    return hip_err(ctx, e, "hipEventCreate(ring)");
  if (!rg.user_ev && (e = hipEventCreateWithFlags(&rg.user_ev, hipEventDisableTiming)) != hipSuccess)
    return hip_err(ctx, e, "hipEventCreate(ring)");
  // the previous session's launch has ended before the slots are cleared
  if ((e = hipStreamSynchronize(rg.stream)) != hipSuccess)
    return hip_err(ctx, e, "hipStreamSynchronize(ring)");
  // sequence numbers and tickets keep growing across the context's sessions,
  // so no line a previous session left anywhere (host slots, the device
  // mirror, a cache) can read as one of this session's batches
  memset(rg.h, 0, kRingHostBytes);
  rg.method = method;
  rg.iters = max_iters;
  rg.et = et_period;
  rg.prec = precision;
  rg.first = rg.next;
  rg.first_frame = rg.frames;
  // the launch follows the work enqueued on the caller's stream so far
  rg.user_stream = hip_stream ? hip_stream : (void *)ctx->stream;
  if ((e = hipEventRecord(rg.user_ev, (hipStream_t)rg.user_stream)) != hipSuccess ||
      (e = hipStreamWaitEvent(rg.stream, rg.user_ev, 0)) != hipSuccess)
    return hip_err(ctx, e, "frame ring: stream order");
  rc = ring_launch(ctx, rg.next, rg.frames);
  if (rc != LDPC_OK) return rc;
  rg.on = true;
  return LDPC_OK;
}

int64_t ldpc_ring_post(ldpc_ctx *ctx, const float *d_in, int64_t cw_stride, int B,
                       uint8_t *d_out_packed, int32_t *d_iters_used_opt,
                       int32_t *d_syn_weight_opt) {
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Ring &rg = ctx->ring;
  if (!rg.on) return set_err(ctx, LDPC_EINVAL, "no frame ring session (ldpc_ring_begin)");
  if (B < 1) return set_err(ctx, LDPC_EINVAL, "B must be >= 1");
  if (!d_in || !d_out_packed) return set_err(ctx, LDPC_EINVAL, "null buffer");
  if (cw_stride < ctx->code.N || cw_stride >= ((int64_t)1 << 40))
    return set_err(ctx, LDPC_EINVAL, "cw_stride must be in [N, 2^40)");
  for (const void *p : {(const void *)d_in, (const void *)d_out_packed, (const void *)d_iters_used_opt,
                        (const void *)d_syn_weight_opt})
    if ((uintptr_t)p >> 48) return set_err(ctx, LDPC_EINVAL, "pointer above 2^48");
  if (rg.frames - rg.first_frame + B >= ((int64_t)1 << 31) || rg.frames + B >= ((int64_t)1 << 47))
    return set_err(ctx, LDPC_EINVAL, "a frame ring session takes < 2^31 frames: end it and begin anew");
  return ring_post_impl(ctx, d_in, cw_stride, B, d_out_packed, d_iters_used_opt, d_syn_weight_opt, 0);
}

int ldpc_ring_wait(ldpc_ctx *ctx, int64_t batch) {
  if (!ctx) return LDPC_EINVAL;
  if (batch < (int64_t)ctx->ring.first || (uint64_t)batch >= ctx->ring.next)
    return set_err(ctx, LDPC_EINVAL, "no such batch in this session");
  return ring_wait_impl(ctx, (uint64_t)batch);
}

int ldpc_ring_end(ldpc_ctx *ctx) {
  if (!ctx) return LDPC_EINVAL;
  ldpc_ctx::Ring &rg = ctx->ring;
  if (!rg.on) return LDPC_OK;
  rg.on = false;
  const int64_t q = ring_post_impl(ctx, nullptr, 0, 0, nullptr, nullptr, nullptr, 1);
  if (q < 0) return (int)q;
  // work the caller enqueues on its stream from now on follows the launch
  hipError_t e = hipStreamWaitEvent((hipStream_t)rg.user_stream, rg.ev, 0);
  if (e != hipSuccess) return hip_err(ctx, e, "frame ring: stream order");
  // the next session's counters, zeroed on the ring's stream once this
  // launch has ended (the caller's stream waits for the launch only)
  if ((e = hipMemsetAsync(rg.d, 0, kRingDevBytes, rg.stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemsetAsync(ring)");
  rg.clean = true;
  return LDPC_OK;
}

int ldpc_ring_info(const ldpc_ctx *ctx, int *launches_out, int *workgroups_out) {
  if (!ctx) return LDPC_EINVAL;
  if (launches_out) *launches_out = ctx->ring.launches;
  if (workgroups_out) *workgroups_out = ctx->ring.workgroups;
  return LDPC_OK;
}

}  // extern "C"
