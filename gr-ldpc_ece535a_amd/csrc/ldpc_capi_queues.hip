// ldpc_capi_queues.hip -- the C ABI of include/ldpc_hip.h: the frame-queue
// counters of the streams that launch on a context, the in-flight stream set
// (ldpc_ctx_streams) with its concurrency probe, and the test hooks.  Owns
// the context's queues group (ldpc_ctx.hpp).
#include <chrono>

#include "ldpc_aux.hpp"
#include "ldpc_ctx.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Queues::release() {
  for (hipStream_t t : tp_streams) {
    (void)hipStreamSynchronize(t);
    (void)hipStreamDestroy(t);
  }
  tp_streams.clear();
  free_device(d_probe);
  free_device(d_tickets);
  list.clear();
}

namespace ldpc {
namespace capi {

bool ensure_tickets(ldpc_ctx *ctx, const char *&failed, hipError_t &e) {
  if (ctx->queues.d_tickets) return !failed;
  const std::vector<uint32_t> zeros((size_t)kTicketSlots * kTicketStride, 0);
  return upload(&ctx->queues.d_tickets, zeros, "upload(tickets)", failed, e);
}

int stream_queue(ldpc_ctx *ctx, void *st, size_t &q) {
  hipError_t e;
  std::vector<ldpc_ctx::Queues::Queue> &list = ctx->queues.list;
  q = 0;
  while (q < list.size() && list[q].stream != st) ++q;
  if (q == list.size()) {
    if (q == kTicketSlots) {
      // more streams than counters: drain the device, start every queue over.
      // The memset runs on the null stream, which non-blocking streams are
      // not ordered after: wait for it before any stream launches again.
      if ((e = hipDeviceSynchronize()) != hipSuccess ||
          (e = hipMemset(ctx->queues.d_tickets, 0,
                         (size_t)kTicketSlots * kTicketStride * sizeof(uint32_t))) != hipSuccess ||
          (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_err(ctx, e, "ticket reset");
      list.clear();
      q = 0;
    }
    // slots are handed out in order from zeroed memory (creation, reset)
    list.push_back({st, 0u});
  }
  return LDPC_OK;
}

// The host's half of the frame-queue protocol (ldpc_kernels.hpp
// DecodeArgs::ticket; the device's: ldpc_wgframe.hpp wg_next_frame and the
// small-code kernels' claims).  The counter only grows, and base is its value
// when the next launch on the stream starts: a launch whose frame indices are
// counter - base stays below B only if every launch before it was committed
// with exactly what it added.
int bind_queue(ldpc_ctx *ctx, void *st, int max_iters, ldpc::DecodeArgs &a, size_t &q) {
  const int rc = stream_queue(ctx, st, q);
  if (rc != LDPC_OK) return rc;
  a.ticket = ctx->queues.d_tickets + q * kTicketStride;
  a.ticket_base = ctx->queues.list[q].base;
  a.waves = 0;  // the launcher's
  // short frames (iteration cap <= 10): fixed frame stride, no queue atomics
  // (DecodeArgs::static_stride)
  a.static_stride = max_iters <= 10 ? 1 : 0;
  return LDPC_OK;
}

void commit_queue(ldpc_ctx *ctx, size_t q, uint32_t advance) {
  ctx->queues.list[q].base += advance;
}

}  // namespace capi
}  // namespace ldpc

extern "C" {

int ldpc_ctx_streams(ldpc_ctx *ctx, int n, void **streams_out) {
  if (!ctx || n < 1 || n > 16 || !streams_out)
    return set_err(ctx, LDPC_EINVAL, "n must be in [1, 16] with an output array");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  uint32_t *&d_probe = ctx->queues.d_probe;
  std::vector<hipStream_t> &set = ctx->queues.tp_streams;
  if (!d_probe && (e = hipMalloc((void **)&d_probe, 256)) != hipSuccess)
    return hip_err(ctx, e, "hipMalloc(probe)");
  // Which hardware queue a stream lands on (GPU_MAX_HW_QUEUES of them) depends
  // on every stream the process made before it; two streams on one queue run
  // their launches one after the other.  A candidate joins the set only if a
  // probe pair runs concurrently with every member (both ways round); the
  // others are kept until the set is complete (so the next candidate lands
  // elsewhere), then freed, and the finished set is probed once more.
  // Measured (profiles/round5/inflight_bimodal.txt): a stream's FIRST launch
  // can run beside a launch on a stream that shares its queue, so a probe
  // that is a candidate's first use passed sets whose streams then ran one
  // after the other -- one process in four at 0.72x the in-flight rate.  Every
  // candidate now makes a launch of its own (and waits for it) before it is
  // probed, and a probe waits up to 5 ms.  A new stream lands on the queue
  // fewest streams use, so when the process's streams sit unevenly on its
  // queues (a test process that made dozens) the missing queue is reached
  // only after the others have taken the rejected candidates: up to 16 per
  // wanted stream are tried.
  int rc = LDPC_OK;
  if (set.size() < (size_t)n) {
    // the probes should see only each other: the context's own work is waited
    // for (its stream, the frame ring's, the set so far; a window server is
    // ended first) -- not the device: other contexts of the process (other
    // blocks of a flowgraph) keep running.  Their work can hold a probe back
    // past its timeout; the candidate is then rejected and another tried.
    serve_stop(ctx);
    auto own_idle = [&]() {
      hipError_t r = hipStreamSynchronize(ctx->stream);
      if (r == hipSuccess && ctx->ring.stream) r = hipStreamSynchronize(ctx->ring.stream);
      for (hipStream_t t : set)
        if (r == hipSuccess) r = hipStreamSynchronize(t);
      return r;
    };
    if ((e = own_idle()) != hipSuccess) return hip_err(ctx, e, "hipStreamSynchronize");
    // total probing is bounded: ~0.5 s, after which the set is what it is
    const auto t_start = std::chrono::steady_clock::now();
    auto over = [&]() {
      return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > 0.5;
    };
    auto concurrent = [&](hipStream_t a, hipStream_t c, bool &ok) {
      uint32_t seen = 0;
      if ((e = hipMemset(d_probe, 0, 8)) != hipSuccess ||
          ldpc::launch_probe_pair(d_probe, 500000 /* 5 ms */, a, c) != 0 ||
          (e = hipStreamSynchronize(a)) != hipSuccess || (e = hipStreamSynchronize(c)) != hipSuccess ||
          (e = hipMemcpy(&seen, d_probe + 1, 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_err(ctx, e, "stream probe");
      ok = seen == 1u;
      return LDPC_OK;
    };
    auto both_ways = [&](hipStream_t a, hipStream_t c, bool &ok) {
      int r = concurrent(a, c, ok);
      if (r == LDPC_OK && ok) r = concurrent(c, a, ok);
      return r;
    };
    auto fresh = [&](hipStream_t &c) {
      c = nullptr;
      if ((e = hipStreamCreateWithFlags(&c, hipStreamNonBlocking)) != hipSuccess)
        return hip_err(ctx, e, "hipStreamCreate");
      if (ldpc::launch_probe_touch(d_probe + 8, c) != 0 ||
          (e = hipStreamSynchronize(c)) != hipSuccess) {
        (void)hipStreamDestroy(c);
        c = nullptr;
        return hip_err(ctx, e, "stream probe");
      }
      return LDPC_OK;
    };
    // members handed out by an earlier call stay (their callers hold them)
    const size_t held = set.size();
    for (int attempt = 0; attempt < 3 && rc == LDPC_OK; ++attempt) {
      std::vector<hipStream_t> spare;
      // (more streams than the process has hardware queues cannot all be
      // concurrent: after a few candidates the set's streams are handed out
      // again)
      for (int tries = 0; (int)set.size() < n && tries < 16 * n && (set.empty() || !over());
           ++tries) {
        hipStream_t c = nullptr;
        if ((rc = fresh(c)) != LDPC_OK) break;
        bool ok = true;
        for (hipStream_t a : set) {
          rc = both_ways(a, c, ok);
          if (rc != LDPC_OK || !ok) break;
        }
        (ok && rc == LDPC_OK ? set : spare).push_back(c);
        if (rc != LDPC_OK) break;
      }
      for (hipStream_t t : spare) (void)hipStreamDestroy(t);
      if (rc != LDPC_OK) break;
      // freeing a stream can release its hardware queue, and for a few ms
      // after that probes read concurrent pairs as shared: let it settle
      if ((e = own_idle()) != hipSuccess) return hip_err(ctx, e, "hipStreamSynchronize");
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
      // the finished set, once more; one that fails is made again, and after
      // three tries the last one stays (a set, even a slower one, rather than
      // an error)
      bool all = true;
      for (size_t i = 0; i < set.size() && all && rc == LDPC_OK; ++i)
        for (size_t j = i + 1; j < set.size() && all && rc == LDPC_OK; ++j)
          rc = both_ways(set[i], set[j], all);
      if (rc != LDPC_OK || all || attempt == 2 || over()) break;
      for (size_t i = held; i < set.size(); ++i) (void)hipStreamDestroy(set[i]);
      set.resize(held);
    }
    if (rc != LDPC_OK) return rc;
  }
  if (set.empty()) return set_err(ctx, LDPC_EDEVICE, "no stream");
  const size_t m = set.size();
  for (int i = 0; i < n; ++i) streams_out[i] = (void *)set[(size_t)i % m];
  // the distinct streams handed out (the set's concurrent ones, at most n)
  return (int)std::min<size_t>(m, (size_t)n);
}

int ldpc_test_hook(ldpc_ctx *ctx, int op, int64_t arg) {
  if (!ctx) return LDPC_EINVAL;
  switch (op) {
    case LDPC_TEST_SERVE_UNCHECKED:
      ctx->serve.test_skip_check = true;
      return LDPC_OK;
    case LDPC_TEST_SERVE_EPOCH:
      // epochs only grow within a session (a launch serves epochs above its start)
      if (arg < (int64_t)ctx->serve.epoch || arg >= (int64_t)ldpc::kServeEpochLimit)
        return set_err(ctx, LDPC_EINVAL, "epoch must be in [current, kServeEpochLimit)");
      ctx->serve.epoch = (uint32_t)arg;
      return LDPC_OK;
    case LDPC_TEST_SERVE_EPOCH_NOW:
      return (int)ctx->serve.epoch;
    case LDPC_TEST_STREAM_OVERLAP: {
      // streams i = arg >> 8 and j = arg & 255 of the in-flight set: a 0.2 ms
      // spin on each, 1 if the two spins' device-clock intervals intersect
      const std::vector<hipStream_t> &set = ctx->queues.tp_streams;
      const size_t i = (size_t)(arg >> 8) & 255u, j = (size_t)arg & 255u;
      if (i >= set.size() || j >= set.size())
        return set_err(ctx, LDPC_EINVAL, "no such stream in the set");
      hipError_t e;
      if (!ctx->queues.d_probe && (e = hipMalloc((void **)&ctx->queues.d_probe, 256)) != hipSuccess)
        return hip_err(ctx, e, "hipMalloc(probe)");
      uint64_t *st = reinterpret_cast<uint64_t *>(ctx->queues.d_probe) + 8, h[4] = {0, 0, 0, 0};
      if (ldpc::launch_stamp(st, 20000, set[i]) != 0 ||
          ldpc::launch_stamp(st + 2, 20000, set[j]) != 0 ||
          (e = hipStreamSynchronize(set[i])) != hipSuccess ||
          (e = hipStreamSynchronize(set[j])) != hipSuccess ||
          (e = hipMemcpy(h, st, sizeof h, hipMemcpyDeviceToHost)) != hipSuccess)
        return set_err(ctx, LDPC_EDEVICE, "stream overlap probe");
      return h[2] < h[1] && h[0] < h[3] ? 1 : 0;
    }
    default:
      return set_err(ctx, LDPC_EINVAL, "unknown test hook");
  }
}

}  // extern "C"
