// ldpc_capi_serve.hip -- the C ABI of include/ldpc_hip.h: the host side of the
// window server (ldpc_serve.hip, ldpc_serve_*).  One persistent launch polls a
// round word in mapped pinned memory; the host posts a round's keys and spins
// on the result granules.  Owns the context's serve group (ldpc_ctx.hpp).
#include <stdio.h>

#include <chrono>

#include "ldpc_ctx.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Serve::release() {
  free_pinned(h);
  free_device(d_ctl);
  free_device(d_keys);
  cap = 0;
}

namespace {

// Mapped pinned memory: the round word (its own 256 bytes), the keys, the
// result granules.
size_t srv_keys_off() { return 256; }
size_t srv_res_off(int64_t cap) { return 256 + (((size_t)cap * 8 + 255) & ~(size_t)255); }
size_t srv_bytes(int64_t cap) { return srv_res_off(cap) + (size_t)cap * 8; }

// Posts round word (epoch << 32) | B after the keys (x86 stores are ordered;
// the device reads the keys only after it has seen the round word).
// Round word (ldpc_kernels.hpp): (epoch << 32) | (session << 20) | B; the
// session tells a launch still polling after its quit round was overwritten
// that the rounds are no longer its own.
void serve_post(ldpc_ctx *ctx, uint32_t B) {
  ldpc_ctx::Serve &s = ctx->serve;
  ++s.epoch;  // < 2^23: ldpc_serve_begin restarts the epochs well before
  __atomic_store_n(reinterpret_cast<uint64_t *>(s.h),
                   ((uint64_t)s.epoch << 32) | ((uint64_t)(s.launches & 0xFFF) << 20) |
                       (B & ldpc::kServeB),
                   __ATOMIC_RELEASE);
}

// Launches the window server for the context's parameters on its stream
// (ctl zeroed first: it must read below every epoch the launch serves).
// repost_n >= 0 (a relaunch after the old launch's deadline): the round the
// host is waiting on, repost_n windows, is posted again with the NEW session
// before the launch, so the new poller never sees the old session's word for
// it and quits (the host used to post after the launch).
int serve_launch(ldpc_ctx *ctx, int repost_n = -1) {
  ldpc_ctx::Serve &s = ctx->serve;
  hipError_t e;
  if (!s.d_ctl || !s.d_keys || !s.h)
    return set_err(ctx, LDPC_EINVAL, "window server buffers missing");
  if ((e = hipSetDevice(ctx->device)) != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  if ((e = hipMemsetAsync(s.d_ctl, 0, ldpc::kServeCtlBytes, ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemsetAsync(server ctl)");
  void *dh = nullptr;
  if ((e = hipHostGetDevicePointer(&dh, s.h, 0)) != hipSuccess)
    return hip_err(ctx, e, "hipHostGetDevicePointer(server)");
  ldpc::ServeArgs sa{};
  sa.round = (const uint64_t *)dh;
  sa.keys = (const int64_t *)((uint8_t *)dh + srv_keys_off());
  sa.res = (uint64_t *)((uint8_t *)dh + srv_res_off(s.cap));
  sa.dkeys = s.d_keys;
  sa.ctl = s.d_ctl;
  sa.span = ctx->stage.span_samples;
  const char *dl = getenv("LDPC_SERVE_DEADLINE_MS");
  sa.deadline = (uint64_t)((dl ? atof(dl) : 200.0) * 1e5);  // 100 MHz ticks
  s.launches += 1;  // this launch's session: the rounds posted from now on
  sa.session = (uint32_t)s.launches;
  if (repost_n >= 0) {
    s.epoch -= 1;  // the launch serves epochs above start_epoch
    sa.start_epoch = s.epoch;
    serve_post(ctx, (uint32_t)repost_n);  // the same round (epoch, key tags), the new session
  } else {
    sa.start_epoch = s.epoch;
  }
  // decoder workgroups per CU (capped by occupancy); 0 = as many as fit
  const char *pc = getenv("LDPC_SERVE_BLOCKS_PER_CU");
  sa.blocks_per_cu = pc ? atoi(pc) : 0;
  s.debug = getenv("LDPC_SERVE_DEBUG") != nullptr;  // (read per launch)
  sa.debug = s.debug ? 1 : 0;
  int wg = 0;
  ldpc::DecodeArgs a{};
  a.in = (const float *)ctx->stage.d_span;
  a.cw_stride = ctx->code.N;
  a.elem_stride = 1;
  a.polarity = 1.0f;
  a.max_iters = s.iters;
  a.et_period = 1;
  const int rc = ldpc::launch_serve(code_view(ctx), a, sa, s.method, s.prec, ctx->slots, ctx->nw,
                                    ctx->device, ctx->stream, &wg);
  s.workgroups = wg;
  if (rc == -2) return set_err(ctx, LDPC_EUNSUPPORTED, "no window server for this code shape");
  if (rc != 0) return hip_err(ctx, hipGetLastError(), "window server launch");
  return LDPC_OK;
}

// Starts the epochs over (a new session): the running launch, if any, has
// finished; host keys and results and the device key copies are cleared, so
// no slot carries a tag from before the restart.
int serve_reset_epochs(ldpc_ctx *ctx) {
  ldpc_ctx::Serve &s = ctx->serve;
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return hip_err(ctx, e, "hipStreamSynchronize(server)");
  memset(s.h, 0, srv_bytes(s.cap));
  if ((e = hipMemsetAsync(s.d_keys, 0, (size_t)s.cap * 8, ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemsetAsync(server keys)");
  s.epoch = 0;
  return LDPC_OK;
}

}  // namespace

namespace ldpc {
namespace capi {

void serve_stop_running(ldpc_ctx *ctx) {
  serve_post(ctx, ldpc::kServeB);
  ctx->serve.serving = false;
  (void)hipStreamSynchronize(ctx->stream);
}

}  // namespace capi
}  // namespace ldpc

extern "C" {

int ldpc_serve_begin(ldpc_ctx *ctx, int method, int max_iters, int precision, int max_windows) {
  int rc = check_decode_args(ctx, method, max_iters, 1, precision, 1, 1, ctx ? ctx->code.N : 1);
  if (rc != LDPC_OK) return rc;
  ldpc_ctx::Serve &s = ctx->serve;
  if (ctx->onchip.on)
    return set_err(ctx, LDPC_EUNSUPPORTED,
                   "the window server does not run on an on-chip context (small-code kernels "
                   "only); use ldpc_decode_windows");
  if (ctx->graph.on || ctx->code.KB > 4 || (method != 0 && method != 1))
    return set_err(ctx, LDPC_EUNSUPPORTED,
                   "the window server takes min-sum / sum-product on small codes with KB <= 4");
  if (ctx->stage.span_samples <= 0)
    return set_err(ctx, LDPC_EINVAL, "no staged span (ldpc_stage_span)");
  if (max_windows < 1 || max_windows > (1 << 19))
    return set_err(ctx, LDPC_EINVAL, "max_windows must be in [1, 2^19]");
  if (s.serving) {
    if (s.method == method && s.iters == max_iters && s.prec == precision && s.cap >= max_windows)
      return LDPC_OK;
    serve_stop(ctx);
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  if (!s.d_ctl && (e = hipMalloc((void **)&s.d_ctl, ldpc::kServeCtlBytes)) != hipSuccess)
    return hip_err(ctx, e, "hipMalloc(server ctl)");
  // a new buffer (or epochs near the end of their range) starts the epochs over:
  // the previous launch has finished first
  if (s.cap < max_windows || s.epoch >= ldpc::kServeEpochLimit) {
    (void)hipStreamSynchronize(ctx->stream);
    if (s.cap < max_windows) {
      free_pinned(s.h);
      free_device(s.d_keys);
      s.cap = 0;
      const int64_t cap = std::max<int64_t>(max_windows, 4096);
      if ((e = hipHostMalloc((void **)&s.h, srv_bytes(cap),
                             hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
        return hip_err(ctx, e, "hipHostMalloc(server)");
      if ((e = hipMalloc((void **)&s.d_keys, (size_t)cap * 8)) != hipSuccess)
        return hip_err(ctx, e, "hipMalloc(server keys)");
      s.cap = cap;
    }
    if ((rc = serve_reset_epochs(ctx)) != LDPC_OK) return rc;
  }
  s.method = method;
  s.iters = max_iters;
  s.prec = precision;
  rc = serve_launch(ctx);
  if (rc != LDPC_OK) return rc;
  s.serving = true;
  return LDPC_OK;
}

int ldpc_serve_windows(ldpc_ctx *ctx, const int64_t *win, int B, uint8_t *out_packed,
                       int32_t *syn_weight_opt) {
  if (!ctx) return LDPC_EINVAL;
  ldpc_ctx::Serve &s = ctx->serve;
  if (!s.serving) return set_err(ctx, LDPC_EINVAL, "no window server running (ldpc_serve_begin)");
  if (B < 0) return set_err(ctx, LDPC_EINVAL, "B < 0");
  if (B == 0) return LDPC_OK;
  if (!win || !out_packed) return set_err(ctx, LDPC_EINVAL, "null buffer");
  const int N = ctx->code.N, KB = ctx->code.KB;
  const int64_t span_samples = ctx->stage.span_samples;
  // (ldpc_test_hook 1 skips this check once, so that the device's own check
  // of every key -- ldpc_serve.hip key_fault -- can be exercised)
  const bool host_check = !s.test_skip_check;
  s.test_skip_check = false;
  for (int b = 0; b < B; ++b)
    if (win[b] < 0 || win[b] >= ((int64_t)1 << 40) ||
        (host_check && (win[b] >> 1) + N > span_samples))
      return set_err(ctx, LDPC_EINVAL, "window outside the staged span");
  int device_fault = 0;  // a granule that carries no decode (kServeBadKey / kServeLostKey)
  int64_t fault_key = 0;
  int64_t *keys = (int64_t *)(s.h + srv_keys_off());
  const uint64_t *res = (const uint64_t *)(s.h + srv_res_off(s.cap));
  const double timeout_s = 10.0;
  for (int b0 = 0; b0 < B; b0 += (int)s.cap) {
    const int n = (int)std::min<int64_t>(s.cap, B - b0);
    // epochs stay below kServeEpochLimit (result tags are epoch mod 2^23, and a
    // tag that wrapped would match a stale slot): a session that reaches it is
    // ended and started over before this round
    if (s.epoch + 2 >= ldpc::kServeEpochLimit) {
      serve_stop(ctx);
      int rc = serve_reset_epochs(ctx);
      if (rc == LDPC_OK) rc = serve_launch(ctx);
      if (rc != LDPC_OK) return rc;
      s.serving = true;
    }
    // each key carries the epoch it is posted with (mod 2^24), so the poller
    // can tell a slot it read before this round's write (ldpc_serve.hip)
    const uint64_t ktag = (uint64_t)((s.epoch + 1) & 0xFFFFFFu) << 40;
    for (int b = 0; b < n; ++b) keys[b] = (int64_t)((uint64_t)win[b0 + b] | ktag);
    serve_post(ctx, (uint32_t)n);
    s.rounds += 1;
    const uint32_t tag = s.epoch & 0x7FFFFFu;
    const auto t0 = std::chrono::steady_clock::now();
    auto t_first = t0;
    int relaunches = 0;
    for (int b = 0; b < n; ++b) {
      if (b == 1 && s.debug) t_first = std::chrono::steady_clock::now();
      uint64_t g;
      for (uint32_t spins = 1;; ++spins) {
        g = __atomic_load_n(res + b, __ATOMIC_ACQUIRE);
        if ((uint32_t)(g >> 41) == tag) break;
        if ((spins & 0xFFFu) == 0) {
          // the launch ended (its deadline passed between rounds): start another
          const hipError_t q = hipStreamQuery(ctx->stream);
          if (q == hipSuccess) {
            if (s.debug) {
              uint64_t c[8] = {0}, c0 = 0;
              uint32_t census = 0;
              (void)hipMemcpy(&c0, s.d_ctl, 8, hipMemcpyDeviceToHost);
              (void)hipMemcpy(&census, s.d_ctl + 16 * ldpc::kServeCopies, 4, hipMemcpyDeviceToHost);
              (void)hipMemcpy(c, s.d_ctl + 16 * (ldpc::kServeCopies + 1), sizeof c,
                              hipMemcpyDeviceToHost);
              fprintf(stderr,
                      "ldpc_serve: launch %d ended before round %u (B %d, result %d of them "
                      "in): ctl %016llx census %u, poller exit %llu on round word %016llx, "
                      "host round word %016llx; decoder round starts %llu (g0 saw %016llx), "
                      "mw results %llu\n",
                      s.launches, s.epoch, n, b, (unsigned long long)c0, census,
                      (unsigned long long)c[0], (unsigned long long)c[1],
                      (unsigned long long)*(const uint64_t *)s.h, (unsigned long long)c[2],
                      (unsigned long long)c[3], (unsigned long long)c[4]);
            }
            if (++relaunches > 4) {
              s.serving = false;
              return set_err(ctx, LDPC_ETIMEOUT, "the window server keeps ending before its round");
            }
            const int rc = serve_launch(ctx, n);  // the same round, posted for the new session
            if (rc != LDPC_OK) {
              s.serving = false;
              return rc;
            }
          } else if (q != hipErrorNotReady) {
            s.serving = false;
            return hip_err(ctx, q, "window server");
          }
          if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
            serve_stop(ctx);
            return set_err(ctx, LDPC_ETIMEOUT, "a window server round passed its timeout");
          }
        }
      }
      const uint32_t pk = (uint32_t)g, wt = (uint32_t)(g >> 32) & 511u;
      if (wt == ldpc::kServeBadKey || wt == ldpc::kServeLostKey) {
        if (!device_fault) {
          device_fault = (int)wt;
          fault_key = win[b0 + b];
        }
        continue;  // (the round's other results are still collected)
      }
      for (int j = 0; j < KB; ++j) out_packed[(size_t)(b0 + b) * KB + j] = (uint8_t)(pk >> (8 * j));
      if (syn_weight_opt) syn_weight_opt[b0 + b] = (int32_t)wt;
    }
    if (s.debug) {  // device-side split of the round (100 MHz ticks)
      const double host_us =
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6;
      const double first_us = std::chrono::duration<double>(t_first - t0).count() * 1e6;
      uint64_t c[9] = {0};
      uint64_t *dg = s.d_ctl + 16 * (ldpc::kServeCopies + 1);
      (void)hipMemcpy(c, dg, sizeof c, hipMemcpyDeviceToHost);
      const uint64_t zero[2] = {0, 0};
      (void)hipMemcpy(dg + 6, zero, sizeof zero, hipMemcpyHostToDevice);
      // (only the one-wave form of big rounds does not time its decoders)
      if (c[6] >= c[5] && c[7] >= c[5] && c[5] >= c[8]) {
        s.dbg[0] += 1;
        s.dbg[1] += host_us;
        s.dbg[2] += 1e-2 * (double)(c[5] - c[8]);
        s.dbg[3] += 1e-2 * (double)(c[6] - c[5]);
        s.dbg[4] += 1e-2 * (double)(c[7] - c[5]);
        s.dbg[5] += n > 1 ? first_us : host_us;
      }
    }
  }
  if (device_fault) {
    char buf[200];
    snprintf(buf, sizeof buf,
             "window server: %s (window key %lld, span of %lld samples); the window was not "
             "decoded",
             device_fault == (int)ldpc::kServeBadKey
                 ? "the device refused a window key outside the staged span"
                 : "a window key never reached the device within the deadline",
             (long long)fault_key, (long long)span_samples);
    return set_err(ctx, LDPC_EDEVICE, buf);
  }
  return LDPC_OK;
}

int ldpc_serve_end(ldpc_ctx *ctx) {
  if (!ctx) return LDPC_EINVAL;
  ldpc_ctx::Serve &s = ctx->serve;
  if (s.debug && s.dbg[0] > 0) {
    fprintf(stderr,
            "ldpc_serve: %.0f rounds: host %.1f us per round; poller: sight to publication %.1f "
            "us; from the publication: last key read %.1f us, last result stored %.1f us; host: "
            "first result seen %.1f us after the post (mean over rounds)\n",
            s.dbg[0], s.dbg[1] / s.dbg[0], s.dbg[2] / s.dbg[0], s.dbg[3] / s.dbg[0],
            s.dbg[4] / s.dbg[0], s.dbg[5] / s.dbg[0]);
    for (double &d : s.dbg) d = 0;
    uint32_t census = 0;
    (void)hipMemcpy(&census, s.d_ctl + 16 * ldpc::kServeCopies, 4, hipMemcpyDeviceToHost);
    fprintf(stderr, "ldpc_serve: %u of %d decoder workgroups started\n", census, s.workgroups);
  }
  if (s.serving) {  // the launch finishes on its own; the stream orders what follows
    serve_post(ctx, ldpc::kServeB);
    s.serving = false;
  }
  return LDPC_OK;
}

}  // extern "C"
