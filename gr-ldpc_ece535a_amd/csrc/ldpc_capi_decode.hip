// ldpc_capi_decode.hip -- the C ABI of include/ldpc_hip.h: decodes.  Argument
// checks, the kernels' views of a context, the large-code workspace, kernel
// dispatch for device-resident frames, and the staged paths on top of it
// (host buffers, windows of one sample span).  Owns the context's stage group
// and the workspace of its graph group (ldpc_ctx.hpp).
#include <stdio.h>

#include <chrono>

#include "ldpc_arena.hpp"
#include "ldpc_aux.hpp"
#include "ldpc_ctx.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Stage::release() {
  free_device(d);
  free_pinned(h);
  free_device(d_span);
  free_pinned(h_win);
  d_bytes = h_bytes = span_bytes = h_win_bytes = 0;
  span_samples = 0;
}

namespace {

int ensure_stage(ldpc_ctx *ctx, size_t bytes) {
  ldpc_ctx::Stage &s = ctx->stage;
  if (bytes <= s.d_bytes) return LDPC_OK;
  if (s.d) {
    (void)hipStreamSynchronize(ctx->stream);
    free_device(s.d);
    s.d_bytes = 0;
  }
  size_t want = std::max(bytes, (size_t)1 << 20);
  hipError_t e = hipMalloc(&s.d, want);
  if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(staging)");
  s.d_bytes = want;
  return LDPC_OK;
}

int ensure_host_stage(ldpc_ctx *ctx, size_t bytes) {
  ldpc_ctx::Stage &s = ctx->stage;
  if (s.h_busy) {  // every writer of the pinned stage comes through here
    (void)hipStreamSynchronize(ctx->stream);
    s.h_busy = false;
  }
  if (bytes <= s.h_bytes) return LDPC_OK;
  if (s.h) {
    (void)hipStreamSynchronize(ctx->stream);
    free_pinned(s.h);
    s.h_bytes = 0;
  }
  size_t want = std::max(bytes, (size_t)1 << 20);
  hipError_t e = hipHostMalloc((void **)&s.h, want, hipHostMallocDefault);
  if (e != hipSuccess) return hip_err(ctx, e, "hipHostMalloc(staging)");
  s.h_bytes = want;
  return LDPC_OK;
}

ldpc::OnchipView onchip_view(const ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc::OnchipView v;
  v.erow = ctx->onchip.d_erow;
  v.ecol = reinterpret_cast<const uint2 *>(ctx->onchip.d_ecol);
  v.rows = ctx->onchip.d_rows;
  v.cols = ctx->onchip.d_cols;
  v.ci = ctx->onchip.d_ci;
  v.ce = ctx->onchip.d_ce;
  v.M = code.M;
  v.N = code.N;
  v.E = code.E;
  v.KB = code.KB;
  v.dc_max = code.dc_max;
  v.dv_max = code.dv_max;
  return v;
}

ldpc::GraphView graph_view(const ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc::GraphView g;
  g.rp = ctx->graph.d_rp;
  g.ci = ctx->graph.d_ci;
  g.cp = ctx->graph.d_cp;
  g.ce = ctx->graph.d_ce;
  g.cr = ctx->graph.d_cr;
  g.M = code.M;
  g.N = code.N;
  g.E = code.E;
  g.KB = code.KB;
  g.dc_max = code.dc_max;
  g.dv_max = code.dv_max;
  return g;
}

ldpc::MsnView msn_view(const ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  const ldpc_ctx::Graph &gr = ctx->graph;
  ldpc::MsnView v;
  v.rdesc = gr.d_msnd[0];
  v.rx = gr.d_msn[0];
  v.cdesc = gr.d_msnd[1];
  v.cx = gr.d_msn[1];
  v.corig = gr.d_msn[2];
  v.cpos = gr.d_msn[3];
  v.M = code.M;
  v.N = code.N;
  v.E = code.E;
  v.KB = code.KB;
  v.dc_max = code.dc_max;
  v.dv_max = code.dv_max;
  v.rs = gr.msn.rs;
  v.cs = gr.msn.cs;
  v.out_var = gr.msn.out_var ? 1 : 0;
  return v;
}

// The large-code workspace, at least `need` bytes.
int ensure_work(ldpc_ctx *ctx, size_t need) {
  ldpc_ctx::Graph &g = ctx->graph;
  if (need <= g.work_bytes) return LDPC_OK;
  if (g.d_work) {
    (void)hipDeviceSynchronize();  // the old workspace may be in use on any stream
    free_device(g.d_work);
    g.work_bytes = 0;
  }
  hipError_t e = hipMalloc(&g.d_work, need);
  if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(graph workspace)");
  g.work_bytes = need;
  return LDPC_OK;
}

// Large-code path: frames in groups that fit the workspace limit, each group
// decoded by launch_graph_decode on `st`.
int decode_graph(ldpc_ctx *ctx, const ldpc::DecodeArgs &a, int method, int precision, void *st) {
  ldpc_ctx::Graph &gr = ctx->graph;
  const ldpc::GraphView g = graph_view(ctx);
  const bool want_post = a.llr != nullptr;
  if (method == 0) {
    // min-sum: narrow chunks, gathered state L2-resident per XCD
    if (!gr.narrow)
      return set_err(ctx, LDPC_EUNSUPPORTED,
                     "large-code min-sum needs M <= " + std::to_string(ldpc::kMsnMaxRows) +
                         " check rows (the narrow-chunk pipeline's limit)");
    const ldpc::MsnView v = msn_view(ctx);
    int C = ldpc::msn_default_chunks();
    const int need_c = (a.B + ldpc::kMsnFrames - 1) / ldpc::kMsnFrames;
    if (need_c < C) C = need_c >= 8 ? (need_c + 7) / 8 * 8 : need_c;
    // ldpc_set_work_limit caps the chunks in flight (at least one; multiples
    // of 8 keep the XCD placement)
    while (C > 1 && ldpc::msn_work_bytes(v, C, precision) > gr.work_limit)
      C = C > 8 && C % 8 == 0 ? C - 8 : C - 1;
    int rc = ensure_work(ctx, ldpc::msn_work_bytes(v, C, precision));
    if (rc != LDPC_OK) return rc;
    if (!gr.h_ctrl) {
      hipError_t e = hipHostMalloc((void **)&gr.h_ctrl, 64, hipHostMallocDefault);
      if (e != hipSuccess) return hip_err(ctx, e, "hipHostMalloc(ctrl)");
    }
    ldpc::MsnWork w;
    ldpc::msn_work_carve(w, gr.d_work, v, C, precision);
    rc = ldpc::launch_graph_decode_msn(v, w, a, precision, gr.h_ctrl, st);
    if (rc == -2) return set_err(ctx, LDPC_EUNSUPPORTED, "code degrees outside the large-code kernels");
    if (rc != 0) return hip_err(ctx, hipGetLastError(), "graph kernel launch");
    return LDPC_OK;
  }
  const size_t per64 = ldpc::graph_work_bytes(g, 64, precision, method, want_post);
  int group = (int)std::min<size_t>((size_t)1 << 30, std::max<size_t>(1, gr.work_limit / per64) * 64);
  group = std::min(group, (a.B + 63) / 64 * 64);
  int rc = ensure_work(ctx, ldpc::graph_work_bytes(g, group, precision, method, want_post));
  if (rc != LDPC_OK) return rc;
  for (int b0 = 0; b0 < a.B; b0 += group) {
    const int nb = std::min(group, a.B - b0);
    ldpc::GraphWork w;
    ldpc::graph_work_carve(w, gr.d_work, g, (nb + 63) / 64 * 64, precision, method, want_post);
    ldpc::DecodeArgs s = a;
    s.in = a.in + (int64_t)b0 * a.cw_stride;
    s.B = nb;
    s.packed = a.packed + (int64_t)b0 * g.KB;
    if (a.bits) s.bits = a.bits + (int64_t)b0 * g.N;
    if (a.iters) s.iters = a.iters + b0;
    if (a.synd) s.synd = a.synd + b0;
    if (a.llr) s.llr = a.llr + (int64_t)b0 * g.N;
    rc = ldpc::launch_graph_decode(g, w, s, method, precision, st);
    if (rc == -2) return set_err(ctx, LDPC_EUNSUPPORTED, "code degrees outside the large-code kernels");
    if (rc != 0) return hip_err(ctx, hipGetLastError(), "graph kernel launch");
  }
  return LDPC_OK;
}

// The window-launch staging area: the span at its start, window lists and
// outputs at its end.  A bigger area moves everything: the staged span is gone.
int ensure_window_stage(ldpc_ctx *ctx, size_t need) {
  ldpc_ctx::Stage &s = ctx->stage;
  if (need <= s.span_bytes) return LDPC_OK;
  if (s.d_span) {
    (void)hipStreamSynchronize(ctx->stream);
    free_device(s.d_span);
    s.span_bytes = 0;
  }
  s.span_samples = 0;
  const size_t want = std::max(need + need / 2, (size_t)4 << 20);
  hipError_t e = hipMalloc(&s.d_span, want);
  if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(window staging)");
  s.span_bytes = want;
  return LDPC_OK;
}

// What follows the span in the window staging area, for B windows: the window
// list, the gathered frames where the large-code kernels need them, the
// packed bytes and the syndrome weights.  Over a null base it measures.
struct WindowTail {
  int64_t *win;
  float *frames;
  uint8_t *packed;
  int32_t *synd;
  size_t bytes;
};

// the span's own region at the start of the area, S samples
size_t span_bytes(int64_t S) {
  ldpc::Arena a;
  a.take<float>((size_t)S);
  return a.bytes();
}

WindowTail window_tail(void *base, size_t B, int N, int KB, bool gather) {
  ldpc::Arena a(base);
  WindowTail t;
  t.win = a.take<int64_t>(B);
  t.frames = gather ? a.take<float>(B * (size_t)N) : nullptr;
  t.packed = a.take<uint8_t>(B * (size_t)KB);
  t.synd = a.take<int32_t>(B);
  t.bytes = a.bytes();
  return t;
}

// S samples in[i * elem_stride] -> pinned host stage -> d_span (enqueued on
// the context's stream; the launches that read it follow on the same stream).
int copy_span(ldpc_ctx *ctx, const float *in, int64_t S, int elem_stride, float *d_span) {
  int rc = ensure_host_stage(ctx, (size_t)S * 4);
  if (rc != LDPC_OK) return rc;
  ldpc_ctx::Stage &s = ctx->stage;
  float *h = s.h;
  if (S >= ((int64_t)1 << 17)) {
    // big spans: gathered by the pool, each piece sent once ready
    if (!s.gather) {
      s.gather.reset(new GatherPool);
      for (int t = 0; t < GatherPool::kThreads; ++t)
        s.gather->th.emplace_back([g = s.gather.get()] { g->worker(); });
    }
    GatherPool &g = *s.gather;
    const int64_t np = (S + GatherPool::kPiece - 1) / GatherPool::kPiece;
    uint64_t gen;
    {
      std::lock_guard<std::mutex> lk(g.mu);
      if (g.ready_cap < np) {
        g.ready.reset(new std::atomic<uint64_t>[np]);
        for (int64_t p = 0; p < np; ++p) g.ready[p].store(0);
        g.ready_cap = np;
      }
      g.in = in;
      g.h = h;
      g.S = S;
      g.stride = elem_stride;
      g.npieces = np;
      g.next.store(0);
      gen = ++g.gen;
    }
    g.cv.notify_all();
    constexpr int64_t per_copy = GatherPool::kCopy / GatherPool::kPiece;
    for (int64_t p = 0; p < np; ++p) {
      while (g.ready[p].load(std::memory_order_acquire) != gen) {
        const int64_t q = g.next.fetch_add(1);  // help while waiting
        if (q < np) {
          g.gather(q);
          g.ready[q].store(gen, std::memory_order_release);
        } else {
          std::this_thread::yield();
        }
      }
      if ((p + 1) % per_copy != 0 && p + 1 != np) continue;
      const int64_t i0 = (p / per_copy) * GatherPool::kCopy, n = std::min(S - i0, GatherPool::kCopy);
      hipError_t e = hipMemcpyAsync(d_span + i0, h + i0, (size_t)n * 4, hipMemcpyHostToDevice,
                                    ctx->stream);
      if (e != hipSuccess) return hip_err(ctx, e, "hipMemcpyAsync(span)");
    }
    s.h_busy = true;
    s.span_samples = S;
    return LDPC_OK;
  }
  // in pieces: each piece's copy to the device runs while the next is gathered
  const int64_t piece = S;
  for (int64_t i0 = 0; i0 < S; i0 += piece) {
    const int64_t i1 = std::min(S, i0 + piece);
    if (elem_stride == 1)
      memcpy(h + i0, in + i0, (size_t)(i1 - i0) * 4);
    else if (elem_stride == 2)  // gr_complex real parts (the block): a constant stride vectorises
      for (int64_t i = i0; i < i1; ++i) h[i] = in[2 * i];
    else
      for (int64_t i = i0; i < i1; ++i) h[i] = in[i * elem_stride];
    hipError_t e = hipMemcpyAsync(d_span + i0, h + i0, (size_t)(i1 - i0) * 4,
                                  hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return hip_err(ctx, e, "hipMemcpyAsync(span)");
  }
  s.h_busy = true;
  s.span_samples = S;
  return LDPC_OK;
}

}  // namespace

namespace ldpc {
namespace capi {

int check_decode_args(ldpc_ctx *ctx, int &method, int max_iters, int et_period, int precision,
                      int B, int elem_stride, int64_t cw_stride) {
  if (!ctx) return LDPC_EINVAL;
  if (method < 0 || method > 3) method = 0;  // general_work :162-164
  if (B < 0) return set_err(ctx, LDPC_EINVAL, "B < 0");
  if ((method == 0 || method == 1) && max_iters < 1)
    return set_err(ctx, LDPC_EINVAL, "max_iters must be >= 1 for min-sum / sum-product");
  if (method == 2 && max_iters < 0) return set_err(ctx, LDPC_EINVAL, "max_iters < 0");
  if (et_period < 1) return set_err(ctx, LDPC_EINVAL, "et_period must be >= 1");
  if (precision != LDPC_PREC_F64 && precision != LDPC_PREC_F32 &&
      precision != LDPC_PREC_F64_LIBM && precision != LDPC_PREC_F64_FAST)
    return set_err(ctx, LDPC_EINVAL, "precision must be one of LDPC_PREC_*");
  if (elem_stride < 1 || cw_stride < 0) return set_err(ctx, LDPC_EINVAL, "bad strides");
  return LDPC_OK;
}

ldpc::CodeView code_view(const ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc::CodeView v;
  v.erow = ctx->small.d_erow;
  v.ecol = ctx->small.d_ecol;
  v.cols = ctx->small.d_cols;
  v.rowmask = ctx->small.d_rowmask;
  v.lane_col = ctx->small.d_lane_col;
  v.col_lane = ctx->small.d_col_lane;
  v.dpos[0] = ctx->small.dpos[0];
  v.dpos[1] = ctx->small.dpos[1];
  v.M = code.M;
  v.N = code.N;
  v.E = code.E;
  v.KB = code.KB;
  v.rs = ctx->rs;
  v.dc_max = code.dc_max;
  v.dv_max = code.dv_max;
  v.dc_min = code.dc_min;
  return v;
}

ldpc::DecodeArgs make_args(const float *d_in, int64_t cw_stride, int elem_stride, float polarity,
                           int B, int max_iters, int et_period, uint8_t *d_packed, uint8_t *d_bits,
                           int32_t *d_iters, int32_t *d_synd, float *d_llr, const int64_t *d_win) {
  ldpc::DecodeArgs a{};
  a.in = d_in;
  a.cw_stride = cw_stride;
  a.elem_stride = elem_stride;
  a.polarity = polarity;
  a.B = B;
  a.pm_half = 0;
  a.win = d_win;
  a.max_iters = max_iters;
  a.et_period = et_period;
  a.packed = d_packed;
  a.bits = d_bits;
  a.iters = d_iters;
  a.synd = d_synd;
  a.llr = d_llr;
  return a;
}

int decode_device_impl(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                       const float *d_in, int64_t cw_stride, int elem_stride, float polarity,
                       int B, int pm_half, uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                       int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                       float *d_llr_out_opt, void *hip_stream, const int64_t *d_win) {
  serve_stop(ctx);
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, B, elem_stride,
                             cw_stride);
  if (rc != LDPC_OK) return rc;
  if (B == 0) return LDPC_OK;
  if (!d_in || !d_out_packed) return set_err(ctx, LDPC_EINVAL, "null device buffer");
  ldpc::DecodeArgs a = make_args(d_in, cw_stride, elem_stride, polarity, B, max_iters, et_period,
                                 d_out_packed, d_out_bits_opt, d_iters_used_opt,
                                 d_syn_weight_opt, d_llr_out_opt, d_win);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  // on-chip contexts: min-sum / sum-product in LDS, the rest as a large code
  const bool onchip = ctx->onchip.on && (method == 0 || method == 1);
  if (ctx->graph.on && !onchip) {
    ldpc_ctx::Graph &gr = ctx->graph;
    const int KB = ctx->code.KB, N = ctx->code.N;
    if (d_win) return set_err(ctx, LDPC_EUNSUPPORTED, "window lists: small-code kernels only");
    // one workspace per context: order this decode after the previous one
    // when it was enqueued on another stream
    if (!gr.done && (e = hipEventCreateWithFlags(&gr.done, hipEventDisableTiming)) != hipSuccess)
      return hip_err(ctx, e, "hipEventCreate");
    if (gr.stream && gr.stream != st &&
        (e = hipStreamWaitEvent((hipStream_t)st, gr.done, 0)) != hipSuccess)
      return hip_err(ctx, e, "hipStreamWaitEvent");
    if (pm_half > 0) {  // the large-code passes run per polarity
      ldpc::DecodeArgs n = a;
      a.B = n.B = pm_half;
      n.polarity = -polarity;
      n.packed += (int64_t)pm_half * KB;
      if (n.bits) n.bits += (int64_t)pm_half * N;
      if (n.iters) n.iters += pm_half;
      if (n.synd) n.synd += pm_half;
      if (n.llr) n.llr += (int64_t)pm_half * N;
      rc = decode_graph(ctx, a, method, precision, st);
      if (rc == LDPC_OK) rc = decode_graph(ctx, n, method, precision, st);
    } else {
      rc = decode_graph(ctx, a, method, precision, st);
    }
    if (rc != LDPC_OK) return rc;
    if ((e = hipEventRecord(gr.done, (hipStream_t)st)) != hipSuccess)
      return hip_err(ctx, e, "hipEventRecord");
    gr.stream = st;
    return LDPC_OK;
  }
  a.pm_half = pm_half;
  size_t q = 0;
  if ((rc = bind_queue(ctx, st, max_iters, a, q)) != LDPC_OK) return rc;
  a.fair_cycles = ctx->small.fair_cycles;
  uint32_t advance = 0;
  if (onchip)
    rc = ldpc::launch_onchip_decode(onchip_view(ctx), a, method, precision, st,
                                    ctx->onchip.resident, &advance);
  else
    rc = ldpc::launch_decode(code_view(ctx), a, method, precision, ctx->slots, ctx->nw,
                             ctx->small.waves_per_cu, ctx->small.schedule, st, &advance);
  if (rc == -2) return set_err(ctx, LDPC_EUNSUPPORTED, "no kernel for this code shape");
  if (rc != 0) return hip_err(ctx, hipGetLastError(), "kernel launch");
  commit_queue(ctx, q, advance);  // B with one frame per claim
  return LDPC_OK;
}

// B_out = B (both false) or 2B (both polarities).  The frames' samples are
// staged through a pinned buffer; for an interleaved gr_complex stream
// (elem_stride 2, even cw_stride) only the real parts are gathered and
// copied, and the kernel reads them densely.  For the fixed-point layered
// decoder precision is unused too.
int decode_host_impl(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                     const float *in, int64_t n_in_floats, int64_t cw_stride, int elem_stride,
                     float polarity, int B, bool both, uint8_t *out_packed, uint8_t *out_bits_opt,
                     int32_t *iters_used_opt, int32_t *syn_weight_opt, float *llr_out_opt,
                     const ldpc::LayeredArith *layered, const ldpc::RmArgs *rm, int64_t rm_total) {
  serve_stop(ctx);
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, B, elem_stride,
                             cw_stride);
  if (rc != LDPC_OK) return rc;
  // a layered decode that will be refused is refused before anything is staged
  if (layered && (rc = layered_arith_ready(ctx, *layered, precision)) != LDPC_OK) return rc;
  if (B == 0) return LDPC_OK;
  if (!in || !out_packed) return set_err(ctx, LDPC_EINVAL, "null buffer");
  const int N = ctx->code.N, KB = ctx->code.KB;
  // a frame's samples: N of them, or what its transmissions hold
  const int64_t n_frame = rm ? rm_total : N;
  const int64_t span = (int64_t)(B - 1) * cw_stride + (n_frame - 1) * elem_stride + 1;
  if (span > n_in_floats) return set_err(ctx, LDPC_EINVAL, "input shorter than the frames read");
  const bool re_only = elem_stride == 2 && cw_stride % 2 == 0;
  const int64_t n_stage = re_only ? (span + 1) / 2 : span;
  const int64_t cw = re_only ? cw_stride / 2 : cw_stride;
  const int es = re_only ? 1 : elem_stride;
  const int BO = both ? 2 * B : B;
  // the device stage in one walk: the input, then the outputs side by side
  // (measured over a null base, carved over the stage)
  float *d_in, *d_llr;
  uint8_t *d_pk, *d_bits;
  int32_t *d_it, *d_sy;
  size_t b_in = 0;
  auto walk = [&](void *base) {
    ldpc::Arena a(base);
    d_in = a.take<float>((size_t)n_stage);
    b_in = a.bytes();
    d_pk = a.take<uint8_t>((size_t)BO * KB);
    d_bits = out_bits_opt ? a.take<uint8_t>((size_t)BO * N) : nullptr;
    d_it = iters_used_opt ? a.take<int32_t>((size_t)BO) : nullptr;
    d_sy = syn_weight_opt ? a.take<int32_t>((size_t)BO) : nullptr;
    d_llr = llr_out_opt ? a.take<float>((size_t)BO * N) : nullptr;
    return a.bytes();
  };
  const size_t b_all = walk(nullptr);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  rc = ensure_stage(ctx, b_all);
  if (rc != LDPC_OK) return rc;
  // the pinned stage carries the input in and, after the kernel (stream
  // order), every output back in one copy of the adjacent device outputs
  const size_t b_out = b_all - b_in;
  rc = ensure_host_stage(ctx, std::max((size_t)n_stage * 4, b_out));
  if (rc != LDPC_OK) return rc;
  walk(ctx->stage.d);
  float *h = ctx->stage.h;
  if (re_only)
    for (int64_t i = 0; i < n_stage; ++i) h[i] = in[2 * i];
  else
    memcpy(h, in, (size_t)span * 4);
  if ((e = hipMemcpyAsync(d_in, h, (size_t)n_stage * 4, hipMemcpyHostToDevice, ctx->stream)) !=
      hipSuccess)
    return hip_err(ctx, e, "hipMemcpyAsync(in)");
  if (layered)
    rc = layered_device_impl(ctx, *layered, max_iters, et_period, precision, d_in, cw, es,
                             polarity, BO, d_pk, d_bits, d_it, d_sy, d_llr, ctx->stream, rm);
  else
    rc = decode_device_impl(ctx, method, max_iters, et_period, precision, d_in, cw, es, polarity,
                            BO, both ? B : 0, d_pk, d_bits, d_it, d_sy, d_llr, ctx->stream);
  if (rc != LDPC_OK) return rc;
  if ((e = hipMemcpyAsync(h, d_pk, b_out, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemcpyAsync(out)");
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipStreamSynchronize");
  const char *ho = (const char *)h;
  struct {
    void *dst;
    const void *src;  // on the device; the pinned copy starts at d_pk
    size_t n;
  } back[] = {{out_packed, d_pk, (size_t)BO * KB},
              {out_bits_opt, d_bits, (size_t)BO * N},
              {iters_used_opt, d_it, (size_t)BO * 4},
              {syn_weight_opt, d_sy, (size_t)BO * 4},
              {llr_out_opt, d_llr, (size_t)BO * N * 4}};
  for (auto &c : back)
    if (c.dst) memcpy(c.dst, ho + ((const char *)c.src - (const char *)d_pk), c.n);
  return LDPC_OK;
}

}  // namespace capi
}  // namespace ldpc

extern "C" {

int ldpc_stage_span(ldpc_ctx *ctx, const float *in, int64_t n_in_floats, int elem_stride,
                    int max_windows) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  if (!in || elem_stride < 1 || n_in_floats < 0 || max_windows < 0)
    return set_err(ctx, LDPC_EINVAL, "bad span");
  const int64_t S = (n_in_floats + elem_stride - 1) / elem_stride;
  // room for that many windows' lists and outputs behind the span
  const size_t extra =
      window_tail(nullptr, (size_t)max_windows, ctx->code.N, ctx->code.KB, ctx->graph.on).bytes;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  int rc = ensure_window_stage(ctx, span_bytes(S) + extra);
  if (rc != LDPC_OK) return rc;
  return copy_span(ctx, in, S, elem_stride, (float *)ctx->stage.d_span);
}

// The span goes to ctx->stage.d_span [0, span), then the window list, the
// gathered frames and the outputs.
int ldpc_decode_windows(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                        const float *in, int64_t n_in_floats, int elem_stride, int reuse_span,
                        const int64_t *win, int B, uint8_t *out_packed,
                        int32_t *syn_weight_opt) {
  serve_stop(ctx);
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, B, elem_stride,
                             ctx ? ctx->code.N : 1);
  if (rc != LDPC_OK) return rc;
  if (B == 0) return LDPC_OK;
  if (!in || !win || !out_packed) return set_err(ctx, LDPC_EINVAL, "null buffer");
  ldpc_ctx::Stage &sg = ctx->stage;
  const int N = ctx->code.N, KB = ctx->code.KB;
  const int64_t S = (n_in_floats + elem_stride - 1) / elem_stride;  // samples in the span
  for (int b = 0; b < B; ++b)
    if (win[b] < 0 || (win[b] >> 1) + N > S)
      return set_err(ctx, LDPC_EINVAL, "window outside the input span");
  // the on-chip kernels read each window in place, like the small-code ones;
  // gathered frames: only the large-code kernels need them
  const bool gather = ctx->graph.on && !(ctx->onchip.on && (method == 0 || method == 1));
  const size_t tail_bytes = window_tail(nullptr, (size_t)B, N, KB, gather).bytes;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  rc = ensure_window_stage(ctx, span_bytes(S) + tail_bytes);
  if (rc != LDPC_OK) return rc;
  // pinned: the window list in, then the packed words and syndrome weights
  // out in one copy (d_pk .. d_sy are adjacent in the staging area), so no
  // transfer goes through a pageable bounce: the same tail without the frames
  const size_t h_need = window_tail(nullptr, (size_t)B, N, KB, false).bytes;
  if (h_need > sg.h_win_bytes) {
    if (sg.h_win) {
      (void)hipStreamSynchronize(ctx->stream);
      free_pinned(sg.h_win);
      sg.h_win_bytes = 0;
    }
    const size_t want = std::max(h_need + h_need / 2, (size_t)1 << 16);
    // mapped and coherent: the small-code kernels read the window list and
    // write their outputs here directly (no copy either way; see below)
    if ((e = hipHostMalloc((void **)&sg.h_win, want,
                           hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
      return hip_err(ctx, e, "hipHostMalloc(windows)");
    sg.h_win_bytes = want;
  }
  // the span sits at the start of the staging area; a reused span must be the
  // one staged last, with the same length (then it ends before span_cap)
  const size_t span_cap = sg.span_bytes - tail_bytes;
  float *d_span = (float *)sg.d_span;
  WindowTail dt = window_tail((char *)sg.d_span + span_cap, (size_t)B, N, KB, gather);
  const WindowTail ht = window_tail(sg.h_win, (size_t)B, N, KB, false);
  const auto tnow = []() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  double t0 = sg.profile ? tnow() : 0.0;
  if (!(reuse_span && sg.span_samples == S)) {
    rc = copy_span(ctx, in, S, elem_stride, d_span);
    if (rc != LDPC_OK) return rc;
  }
  if (sg.profile) {
    const double t1 = tnow();
    sg.prof[0] += t1 - t0;
    t0 = t1;
  }
  // the previous call's copy out of h_win has completed (it synchronised)
  memcpy(ht.win, win, (size_t)B * 8);
  // Small codes: the kernel reads the (pinned, mapped) window list and writes
  // its packed bytes and syndrome weights into pinned memory itself -- a few
  // bytes per window over the bus, and no DMA round trip on a launch whose
  // latency is that of one frame
  const bool direct = !ctx->graph.on;
  if (direct) {
    void *dv = nullptr;
    if ((e = hipHostGetDevicePointer(&dv, sg.h_win, 0)) != hipSuccess)
      return hip_err(ctx, e, "hipHostGetDevicePointer(windows)");
    dt = window_tail(dv, (size_t)B, N, KB, false);
  } else if ((e = hipMemcpyAsync(dt.win, ht.win, (size_t)B * 8, hipMemcpyHostToDevice,
                                 ctx->stream)) != hipSuccess) {
    return hip_err(ctx, e, "hipMemcpyAsync(windows)");
  }
  if (gather) {  // the large-code kernels read frames at a fixed stride: gather first
    if (ldpc::launch_gather_windows(d_span, dt.win, B, N, dt.frames, ctx->stream) != 0)
      return set_err(ctx, LDPC_EDEVICE, "gather_windows launch failed");
    rc = decode_device_impl(ctx, method, max_iters, et_period, precision, dt.frames, N, 1, 1.0f,
                            B, 0, dt.packed, nullptr, nullptr, syn_weight_opt ? dt.synd : nullptr,
                            nullptr, ctx->stream);
  } else {  // the small-code kernels read each window in place (DecodeArgs::win)
    rc = decode_device_impl(ctx, method, max_iters, et_period, precision, d_span, N, 1, 1.0f, B,
                            0, dt.packed, nullptr, nullptr, syn_weight_opt ? dt.synd : nullptr,
                            nullptr, ctx->stream, dt.win);
  }
  if (rc != LDPC_OK) return rc;
  // packed bytes alone, or through the syndrome weights behind them
  const size_t out_bytes =
      syn_weight_opt ? (size_t)((uint8_t *)(ht.synd + B) - ht.packed) : (size_t)B * KB;
  if (!direct && (e = hipMemcpyAsync(ht.packed, dt.packed, out_bytes, hipMemcpyDeviceToHost,
                                     ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipMemcpyAsync(out)");
  if (sg.profile) {
    const double t1 = tnow();
    sg.prof[1] += t1 - t0;
    t0 = t1;
  }
  // wait for the launch (polling measured no faster,
  // profiles/round2/block/window_latency.txt)
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    return hip_err(ctx, e, "hipStreamSynchronize");
  if (sg.profile) {
    const double t1 = tnow();
    sg.prof[2] += t1 - t0;
    t0 = t1;
  }
  memcpy(out_packed, ht.packed, (size_t)B * KB);
  if (syn_weight_opt) memcpy(syn_weight_opt, ht.synd, (size_t)B * 4);
  if (sg.profile) {
    sg.prof[3] += tnow() - t0;
    sg.calls += 1;
    sg.windows += B;
    if (sg.trace) {
      static double last[4] = {0, 0, 0, 0};
      fprintf(stderr, "decode_windows B=%d stage %.1f list+launch %.1f wait %.1f results %.1f us\n",
              B, 1e6 * (sg.prof[0] - last[0]), 1e6 * (sg.prof[1] - last[1]),
              1e6 * (sg.prof[2] - last[2]), 1e6 * (sg.prof[3] - last[3]));
      for (int i = 0; i < 4; ++i) last[i] = sg.prof[i];
    }
  }
  return LDPC_OK;
}

int ldpc_decode_device(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                       const float *d_in, int64_t cw_stride, int elem_stride, float polarity,
                       int B, uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                       int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                       float *d_llr_out_opt, void *hip_stream) {
  return decode_device_impl(ctx, method, max_iters, et_period, precision, d_in, cw_stride,
                            elem_stride, polarity, B, 0, d_out_packed, d_out_bits_opt,
                            d_iters_used_opt, d_syn_weight_opt, d_llr_out_opt, hip_stream);
}

int ldpc_decode_strided(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                        const float *in, int64_t n_in_floats, int64_t cw_stride, int elem_stride,
                        float polarity, int B, uint8_t *out_packed, uint8_t *out_bits_opt,
                        int32_t *iters_used_opt, int32_t *syn_weight_opt, float *llr_out_opt) {
  return decode_host_impl(ctx, method, max_iters, et_period, precision, in, n_in_floats,
                          cw_stride, elem_stride, polarity, B, false, out_packed, out_bits_opt,
                          iters_used_opt, syn_weight_opt, llr_out_opt);
}

int ldpc_decode_strided_both(ldpc_ctx *ctx, int method, int max_iters, int et_period,
                             int precision, const float *in, int64_t n_in_floats,
                             int64_t cw_stride, int elem_stride, float polarity, int B,
                             uint8_t *out_packed, int32_t *syn_weight_opt) {
  return decode_host_impl(ctx, method, max_iters, et_period, precision, in, n_in_floats,
                          cw_stride, elem_stride, polarity, B, true, out_packed, nullptr,
                          nullptr, syn_weight_opt, nullptr);
}

int ldpc_decode(ldpc_ctx *ctx, int method, int max_iters, int et_period, int precision,
                const float *llr_re, int B, uint8_t *out_packed, uint8_t *out_bits_opt,
                int32_t *iters_used_opt, int32_t *syn_weight_opt) {
  if (!ctx) return LDPC_EINVAL;
  const int N = ctx->code.N;
  return ldpc_decode_strided(ctx, method, max_iters, et_period, precision, llr_re, (int64_t)B * N,
                             N, 1, 1.0f, B, out_packed, out_bits_opt, iters_used_opt,
                             syn_weight_opt, nullptr);
}

}  // extern "C"
