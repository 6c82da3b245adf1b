// ldpc_capi_layered.hip -- the C ABI of include/ldpc_hip.h: layered min-sum
// (ldpc_layered.hip), float and fixed-point, on per-edge tables or on a
// quasi-cyclic context's base matrix.  The plan in force, its layouts and
// device tables, the refusals in their documented order, the launches and the
// planners.  Owns the context's layered group (ldpc_ctx.hpp).
#include <float.h>
#include <stdio.h>

#include <exception>

#include "ldpc_ctx.hpp"
#include "ldpc_layers.hpp"
#include "ldpc_qc.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Layered::release() {
  for (uint32_t **p : {&d_rows, &d_off, &d_qc_rows, &d_qc_ent}) free_device(*p);
  for (uint16_t **p : {&d_ci, &d_order}) free_device(*p);
  tabs = false;
}

void ldpc_ctx::Crc::release() {
  free_device(d_w);
  free_device(d_rem);
  rem_cap = last_B = 0;
}

namespace {

int largest_layer(const std::vector<int32_t> &layer_of_row, int L) {
  std::vector<int> n((size_t)L, 0);
  int most = 0;
  for (int32_t l : layer_of_row) most = std::max(most, ++n[l]);
  return most;
}

// A new plan is in force: the layouts and the device tables of the float and
// the fixed-point decoder are the old plan's.
void plan_changed(ldpc_ctx *ctx) {
  ctx->layered.ready = ctx->layered.tabs = ctx->layered.q8_ready = false;
}

// The context's plan: the planner's -- on a quasi-cyclic context the block
// rows -- unless the caller has set one.  Host only.
void ensure_layer_plan(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Layered &lay = ctx->layered;
  if (lay.L > 0) return;
  if (code.qc_Z > 0) {
    lay.of_row.resize((size_t)code.M);
    for (int j = 0; j < code.M; ++j) lay.of_row[j] = j / code.qc_Z;
    lay.L = code.qc_mb;
  } else {
    lay.L = ldpc::plan_layers(code.M, code.N, code.rp.data(), code.ci.data(), lay.of_row);
  }
  plan_changed(ctx);
}

// The plan in force is the block rows of a quasi-cyclic context, whoever set it.
bool block_row_plan(const ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  if (code.qc_Z <= 0 || ctx->layered.L != code.qc_mb) return false;
  for (int j = 0; j < code.M; ++j)
    if (ctx->layered.of_row[j] != j / code.qc_Z) return false;
  return true;
}

// The circulant kernels while the block rows of a quasi-cyclic context are the
// plan; the per-edge tables for any other plan and under LDPC_FLAG_QC_TABLES.
bool circulant_route(const ldpc_ctx *ctx) {
  return !ctx->layered.qc_tables && block_row_plan(ctx);
}

// Builds and uploads the tables of the plan in force (first use, or the first
// decode after ldpc_set_layers), for the float and the fixed-point decoder
// alike: the caller has checked that its decoder takes the code on this route.
int upload_layered_tables(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Layered &lay = ctx->layered;
  if (lay.tabs) return LDPC_OK;
  const bool qc = circulant_route(ctx);
  ldpc::LayeredTables t;
  ldpc::QcTables qt;
  if (qc)
    ldpc::qc_build(code.qc_mb, code.qc_nb, code.qc_Z, code.qc_shifts.data(), qt);
  else
    ldpc::layered_build(code.M, code.rp.data(), code.ci.data(), lay.of_row, lay.L, t);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  // decodes that read the previous plan's tables may still run (any stream)
  if ((lay.d_rows || lay.d_qc_rows) && (e = hipDeviceSynchronize()) != hipSuccess)
    return hip_err(ctx, e, "hipDeviceSynchronize");
  lay.release();
  const char *what = nullptr;
  if (qc) {
    upload(&lay.d_qc_rows, qt.rows, "upload(base rows)", what, e);
    upload(&lay.d_qc_ent, qt.ent, "upload(base entries)", what, e);
  } else {
    upload(&lay.d_rows, t.rows, "upload(layered rows)", what, e);
    upload(&lay.d_ci, t.ci, "upload(layered col_idx)", what, e);
    upload(&lay.d_order, t.order, "upload(layered row order)", what, e);
    upload(&lay.d_off, t.off, "upload(layer offsets)", what, e);
  }
  ensure_tickets(ctx, what, e);  // large-code contexts have no frame queues of their own
  if (what) return hip_err(ctx, e, what);
  lay.qc = qc;
  lay.qc_rows = (int)qt.rows.size();
  lay.tabs = true;
  return LDPC_OK;
}

// The float decoder's layouts for the plan in force, and the tables.
int prepare_layered(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Layered &lay = ctx->layered;
  ensure_layer_plan(ctx);
  if (lay.ready) return LDPC_OK;
  const int most = largest_layer(lay.of_row, lay.L);
  ldpc::layered_layout(code.M, code.N, code.E, code.dc_max, lay.L, most, 0, lay.f64);
  const bool f32 = ldpc::layered_layout(code.M, code.N, code.E, code.dc_max, lay.L, most, 1, lay.f32);
  if (!f32) {  // what no precision fits; a code that fits float alone is refused per decode
    char buf[256];
    snprintf(buf, sizeof buf,
             "the code does not fit the layered kernels: a frame needs %d bytes of LDS in float "
             "(%d in double), the limit is %d; M, N, E must be <= %d and check degrees <= %d "
             "(M=%d N=%d E=%d dc_max=%d)",
             lay.f32.frame, lay.f64.frame, ldpc::kLayeredLdsLimit, ldpc::kLayeredIndexMax,
             ldpc::kLayeredDcMax, code.M, code.N, code.E, code.dc_max);
    return set_err(ctx, LDPC_EUNSUPPORTED, buf);
  }
  if (circulant_route(ctx))
    for (ldpc::LayeredLayout *l : {&lay.f64, &lay.f32}) {
      l->staged = 0;  // the base tables are read through the scalar cache
      l->total = l->frame;
    }
  const int rc = upload_layered_tables(ctx);
  if (rc != LDPC_OK) return rc;
  // the kernel, its threads and bytes may differ
  lay.resident[0] = lay.resident[1] = lay.rm_resident[0] = lay.rm_resident[1] = 0;
  for (int *r : ctx->crc.resident) r[ldpc::kLayeredF64] = r[ldpc::kLayeredF32] = 0;
  lay.ready = true;
  return LDPC_OK;
}

// The fixed-point decoder's layout for the plan in force, and the tables.
int prepare_layered_q8(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Layered &lay = ctx->layered;
  ensure_layer_plan(ctx);
  if (lay.q8_ready) return LDPC_OK;
  const bool qc = circulant_route(ctx);
  const bool fits = ldpc::layered_q8_layout(code.M, code.N, code.E, code.dc_max, code.dv_max, lay.L,
                                            largest_layer(lay.of_row, lay.L), qc ? code.qc_Z : 0,
                                            lay.q8);
  if (!fits) {
    char buf[320];
    if (qc)
      snprintf(buf, sizeof buf,
               "the code does not fit the fixed-point layered kernel: a frame needs %d bytes of "
               "LDS, the limit is %d; M, N and the base entries must be <= %d, check degrees <= %d "
               "and bit degrees <= %d (M=%d N=%d E=%d dc_max=%d dv_max=%d)",
               lay.q8.frame, ldpc::kLayeredLdsLimit, ldpc::kLayeredIndexMax, ldpc::kLayeredDcMax,
               ldpc::kLayeredQ8DvMax, code.M, code.N, code.E, code.dc_max, code.dv_max);
    else
      snprintf(buf, sizeof buf,
               "the code does not fit the fixed-point layered kernel on its per-edge tables: a "
               "frame needs %d bytes of LDS, the limit is %d; M, N, E must be <= %d (only the "
               "circulant kernel of a quasi-cyclic context takes E beyond it), check degrees <= %d "
               "and bit degrees <= %d (M=%d N=%d E=%d dc_max=%d dv_max=%d)",
               lay.q8.frame, ldpc::kLayeredLdsLimit, ldpc::kLayeredIndexMax, ldpc::kLayeredDcMax,
               ldpc::kLayeredQ8DvMax, code.M, code.N, code.E, code.dc_max, code.dv_max);
    return set_err(ctx, LDPC_EUNSUPPORTED, buf);
  }
  const int rc = upload_layered_tables(ctx);
  if (rc != LDPC_OK) return rc;
  lay.q8_resident = lay.rm_q8_resident = 0;
  for (int *r : ctx->crc.resident) r[ldpc::kLayeredQ8] = 0;
  lay.q8_ready = true;
  return LDPC_OK;
}

// What a layered decode needs beyond check_decode_args, in the order the
// refusals are documented: no ring session, a scale in (0, 1], tables for the
// plan in force, and a frame that fits at this precision.  The host entry
// point calls it before it stages anything, the device one before it launches.
int layered_ready(ldpc_ctx *ctx, double scale, int precision) {
  if (ctx->ring.on)
    return set_err(ctx, LDPC_EINVAL, "a frame ring session is open (ldpc_ring_end)");
  if (!(scale > 0.0 && scale <= 1.0))
    return set_err(ctx, LDPC_EINVAL, "scale must be finite, in (0, 1]");
  const int rc = prepare_layered(ctx);
  if (rc != LDPC_OK) return rc;
  const ldpc::LayeredLayout &lay = precision == LDPC_PREC_F32 ? ctx->layered.f32 : ctx->layered.f64;
  if (lay.frame > ldpc::kLayeredLdsLimit) {
    char buf[200];
    snprintf(buf, sizeof buf,
             "the code does not fit the layered kernels at this precision: a frame needs %d "
             "bytes of LDS, the limit is %d (M=%d N=%d E=%d)",
             lay.frame, ldpc::kLayeredLdsLimit, ctx->code.M, ctx->code.N, ctx->code.E);
    return set_err(ctx, LDPC_EUNSUPPORTED, buf);
  }
  return LDPC_OK;
}

// The same for a fixed-point layered decode: no ring session, num in [1, 16]
// and a finite llr_scale > 0, then a code that fits on the route in force.
int layered_q8_ready(ldpc_ctx *ctx, const ldpc::LayeredArith &q8) {
  if (ctx->ring.on)
    return set_err(ctx, LDPC_EINVAL, "a frame ring session is open (ldpc_ring_end)");
  if (q8.num < 1 || q8.num > 16) return set_err(ctx, LDPC_EINVAL, "num must be in [1, 16]");
  if (!(q8.llr_scale > 0.0f && q8.llr_scale <= FLT_MAX))
    return set_err(ctx, LDPC_EINVAL, "llr_scale must be finite and > 0");
  return prepare_layered_q8(ctx);
}

// The arithmetic of ldpc_decode_layered* and of ldpc_decode_layered_q8*.
ldpc::LayeredArith float_arith(double scale, int precision) {
  return {precision == LDPC_PREC_F32 ? ldpc::kLayeredF32 : ldpc::kLayeredF64, scale, 0, 0.0f};
}

ldpc::LayeredArith q8_arith(int num, float llr_scale) {
  return {ldpc::kLayeredQ8, 1.0, num, llr_scale};
}

// A rate-matched layered decode of device frames: the plain decode's checks
// (layered_device_impl repeats them: they are cheap and it is the one place
// that states their order), then the call's transmissions.
int rm_checked(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int max_iters, int et_period,
               int precision, int64_t rx_stride, int n_tx, const int32_t *k0, const int32_t *e,
               float unreceived_lci, int B, ldpc::RmArgs &rm, int64_t &total) {
  serve_stop(ctx);
  int method = LDPC_METHOD_LOGDOMAIN;
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, B, 1, rx_stride);
  if (rc != LDPC_OK) return rc;
  if ((rc = layered_arith_ready(ctx, ar, precision)) != LDPC_OK) return rc;
  if ((rc = rate_match_args(ctx, n_tx, k0, e, unreceived_lci, rm, &total)) != LDPC_OK) return rc;
  if (rx_stride < total)
    return set_err(ctx, LDPC_EINVAL,
                   "rx_stride must be >= the sum of E = " + std::to_string(total) + " (got " +
                       std::to_string(rx_stride) + ")");
  return LDPC_OK;
}

int rm_device(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int max_iters, int et_period,
              int precision, const float *d_in, int64_t rx_stride, float polarity, int n_tx,
              const int32_t *k0, const int32_t *e, float unreceived_lci, int B,
              uint8_t *d_out_packed, uint8_t *d_out_bits_opt, int32_t *d_iters_used_opt,
              int32_t *d_syn_weight_opt, float *d_llr_out_opt, void *hip_stream) {
  ldpc::RmArgs rm;
  int64_t total = 0;
  const int rc = rm_checked(ctx, ar, max_iters, et_period, precision, rx_stride, n_tx, k0, e,
                            unreceived_lci, B, rm, total);
  if (rc != LDPC_OK) return rc;
  return layered_device_impl(ctx, ar, max_iters, et_period, precision, d_in, rx_stride, 1,
                             polarity, B, d_out_packed, d_out_bits_opt, d_iters_used_opt,
                             d_syn_weight_opt, d_llr_out_opt, hip_stream, &rm);
}

int rm_host(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int max_iters, int et_period,
            int precision, const float *in, int64_t n_in_floats, int64_t rx_stride,
            float polarity, int n_tx, const int32_t *k0, const int32_t *e, float unreceived_lci,
            int B, uint8_t *out_packed, uint8_t *out_bits_opt, int32_t *iters_used_opt,
            int32_t *syn_weight_opt, float *llr_out_opt) {
  ldpc::RmArgs rm;
  int64_t total = 0;
  const int rc = rm_checked(ctx, ar, max_iters, et_period, precision, rx_stride, n_tx, k0, e,
                            unreceived_lci, B, rm, total);
  if (rc != LDPC_OK) return rc;
  return decode_host_impl(ctx, LDPC_METHOD_LOGDOMAIN, max_iters, et_period, precision, in,
                          n_in_floats, rx_stride, 1, polarity, B, false, out_packed, out_bits_opt,
                          iters_used_opt, syn_weight_opt, llr_out_opt, &ar, &rm, total);
}

// The column degrees of a CSR H: the largest.
int csr_dv_max(int N, int E, const int32_t *ci) {
  std::vector<int32_t> dv((size_t)N, 0);
  int most = 0;
  for (int e = 0; e < E; ++e) most = std::max(most, ++dv[ci[e]]);
  return most;
}

}  // namespace

namespace ldpc {
namespace capi {

// layered_ready or layered_q8_ready, as the arithmetic asks.
int layered_arith_ready(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int precision) {
  return ar.kind == ldpc::kLayeredQ8 ? layered_q8_ready(ctx, ar)
                                     : layered_ready(ctx, ar.scale, precision);
}

// Same inputs, outputs and frame queues as decode_device_impl (the fixed-point
// decoder's precision is LDPC_PREC_F32, unused).
int layered_device_impl(ldpc_ctx *ctx, const ldpc::LayeredArith &ar, int max_iters, int et_period,
                        int precision, const float *d_in, int64_t cw_stride, int elem_stride,
                        float polarity, int B, uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                        int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                        float *d_llr_out_opt, void *hip_stream, const ldpc::RmArgs *rm) {
  serve_stop(ctx);
  int method = LDPC_METHOD_LOGDOMAIN;
  int rc = check_decode_args(ctx, method, max_iters, et_period, precision, B, elem_stride,
                             cw_stride);
  if (rc != LDPC_OK) return rc;
  if ((rc = layered_arith_ready(ctx, ar, precision)) != LDPC_OK) return rc;
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Layered &ly = ctx->layered;
  const bool q8 = ar.kind == ldpc::kLayeredQ8, f32 = ar.kind == ldpc::kLayeredF32;
  const ldpc::LayeredLayout &lay = q8 ? ly.q8 : f32 ? ly.f32 : ly.f64;
  int *resident = rm ? (q8 ? &ly.rm_q8_resident : &ly.rm_resident[f32])
                     : (q8 ? &ly.q8_resident : &ly.resident[f32]);
  if (B == 0) return LDPC_OK;
  if (!d_in || !d_out_packed) return set_err(ctx, LDPC_EINVAL, "null device buffer");
  ldpc::DecodeArgs a = make_args(d_in, cw_stride, elem_stride, polarity, B, max_iters, et_period,
                                 d_out_packed, d_out_bits_opt, d_iters_used_opt,
                                 d_syn_weight_opt, d_llr_out_opt);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  // while a CRC is set the decode is the kernel that checks it, and frame b's
  // remainder goes to word b of the context's array
  ldpc::CrcArgs crc_args{}, *crc = nullptr;
  if (ctx->crc.len > 0) {
    if ((rc = crc_results_room(ctx, B)) != LDPC_OK) return rc;
    crc_args = {ctx->crc.d_w, ctx->crc.A, code.M, ctx->crc.mode == LDPC_CRC_STOP, ctx->crc.d_rem};
    crc = &crc_args;
    resident = &ctx->crc.resident[rm ? 1 : 0][ar.kind];
  }
  size_t q = 0;
  if ((rc = bind_queue(ctx, st, max_iters, a, q)) != LDPC_OK) return rc;
  uint32_t advance = 0;
  int launched;
  if (ly.qc) {
    ldpc::LayeredQcView v;
    v.rows = ly.d_qc_rows;
    v.ent = ly.d_qc_ent;
    v.M = code.M;
    v.N = code.N;
    v.E = code.E;
    v.KB = code.KB;
    v.mb = ly.qc_rows;
    v.Z = code.qc_Z;
    launched = ldpc::launch_layered_decode(v, a, lay, ar, st, resident, &advance, rm, crc);
  } else {
    ldpc::LayeredView v;
    v.rows = ly.d_rows;
    v.ci = ly.d_ci;
    v.order = ly.d_order;
    v.off = ly.d_off;
    v.M = code.M;
    v.N = code.N;
    v.E = code.E;
    v.KB = code.KB;
    v.L = ly.L;
    launched = ldpc::launch_layered_decode(v, a, lay, ar, st, resident, &advance, rm, crc);
  }
  if (launched != 0) return hip_err(ctx, hipGetLastError(), "kernel launch");
  commit_queue(ctx, q, advance);
  if (crc) {
    ctx->crc.last_B = B;
    ctx->crc.last_stream = st;
  }
  return LDPC_OK;
}

int crc_upload(ldpc_ctx *ctx, int len, uint32_t poly, int filler) {
  std::string why;
  if (!ldpc::crc_check(len, poly, &why)) return set_err(ctx, LDPC_EINVAL, "bad CRC: " + why);
  const int A = ldpc::crc_block(ctx->code.M, ctx->code.N, filler, len, &why);
  if (A < 0) return set_err(ctx, LDPC_EINVAL, "bad CRC: " + why);
  ldpc_ctx::Crc &c = ctx->crc;
  if (c.d_w && c.w_len == len && c.poly == poly && c.A == A) {
    c.len = len;
    return LDPC_OK;
  }
  std::vector<uint32_t> w((size_t)A);
  ldpc::crc_weights(len, poly, A, w.data());
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  // decodes that read the previous weights may still run (any stream)
  if (c.d_w && (e = hipDeviceSynchronize()) != hipSuccess)
    return hip_err(ctx, e, "hipDeviceSynchronize");
  uint32_t *d_w = nullptr;
  const char *what = nullptr;
  if (!upload(&d_w, w, "upload(CRC weights)", what, e)) {
    free_device(d_w);
    return hip_err(ctx, e, what);
  }
  free_device(c.d_w);
  c.d_w = d_w;
  c.len = c.w_len = len;
  c.poly = poly;
  c.A = A;
  c.last_B = 0;
  return LDPC_OK;
}

int crc_results_room(ldpc_ctx *ctx, int B) {
  ldpc_ctx::Crc &c = ctx->crc;
  if (B <= c.rem_cap) return LDPC_OK;
  // the decode before this one may still write the array that goes
  hipError_t e = c.d_rem ? hipDeviceSynchronize() : hipSuccess;
  if (e != hipSuccess) return hip_err(ctx, e, "hipDeviceSynchronize");
  free_device(c.d_rem);
  c.rem_cap = c.last_B = 0;
  if ((e = hipMalloc((void **)&c.d_rem, (size_t)B * 4)) != hipSuccess)
    return hip_err(ctx, e, "hipMalloc(CRC results)");
  c.rem_cap = B;
  return LDPC_OK;
}

}  // namespace capi
}  // namespace ldpc

extern "C" {

int ldpc_plan_layers(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int precision,
                     int32_t *layer_of_row_out_opt, int *n_layers_out_opt,
                     int64_t *lds_bytes_out_opt, int *threads_out_opt) {
  clear_create_error();
  if (!valid_csr(M, N, row_ptr, col_idx))
    return set_err(nullptr, LDPC_EINVAL, "CSR H must be M x N (M < N), columns ascending and in range");
  if (precision < 0 || precision > 3)
    return set_err(nullptr, LDPC_EINVAL, "precision must be one of LDPC_PREC_*");
  try {
    std::vector<int32_t> plan;
    const int L = ldpc::plan_layers(M, N, row_ptr, col_idx, plan);
    int dc_max = 0;
    for (int j = 0; j < M; ++j) dc_max = std::max(dc_max, row_ptr[j + 1] - row_ptr[j]);
    ldpc::LayeredLayout lay;
    const bool fits = ldpc::layered_layout(M, N, row_ptr[M], dc_max, L, largest_layer(plan, L),
                                           precision, lay);
    if (layer_of_row_out_opt) std::copy(plan.begin(), plan.end(), layer_of_row_out_opt);
    if (n_layers_out_opt) *n_layers_out_opt = L;
    if (lds_bytes_out_opt) *lds_bytes_out_opt = fits ? lay.total : lay.frame;
    if (threads_out_opt) *threads_out_opt = lay.threads;
    return fits ? 1 : 0;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_ctx_layers(const ldpc_ctx *ctx, int32_t *layer_of_row_out_opt) {
  if (!ctx) return LDPC_EINVAL;
  ensure_layer_plan(const_cast<ldpc_ctx *>(ctx));  // made on first use; contexts are never const objects
  const std::vector<int32_t> &plan = ctx->layered.of_row;
  if (layer_of_row_out_opt) std::copy(plan.begin(), plan.end(), layer_of_row_out_opt);
  return ctx->layered.L;
}

int ldpc_set_layers(ldpc_ctx *ctx, const int32_t *layer_of_row) {
  if (!ctx) return LDPC_EINVAL;
  if (!layer_of_row) {
    ctx->layered.L = 0;
    ensure_layer_plan(ctx);
    return LDPC_OK;
  }
  const ldpc_ctx::Code &code = ctx->code;
  std::string why;
  const int L = ldpc::check_layers(code.M, code.N, code.rp.data(), code.ci.data(), layer_of_row, &why);
  if (L < 0) return set_err(ctx, LDPC_EINVAL, "bad layer plan: " + why);
  ctx->layered.of_row.assign(layer_of_row, layer_of_row + code.M);
  ctx->layered.L = L;
  plan_changed(ctx);
  return LDPC_OK;
}

int ldpc_plan_qc(int mb, int nb, int Z, const int32_t *shifts, int precision,
                 int32_t *row_ptr_out_opt, int32_t *col_idx_out_opt, int64_t *lds_bytes_out_opt,
                 int *threads_out_opt) {
  clear_create_error();
  std::string why;
  if (!ldpc::qc_check(mb, nb, Z, shifts, &why))
    return set_err(nullptr, LDPC_EINVAL, "bad quasi-cyclic code: " + why);
  if (precision < 0 || precision > 3)
    return set_err(nullptr, LDPC_EINVAL, "precision must be one of LDPC_PREC_*");
  try {
    int entries, row_max;
    ldpc::qc_count(mb, nb, shifts, entries, row_max);
    if (row_ptr_out_opt || col_idx_out_opt) {
      std::vector<int32_t> rp, ci;
      ldpc::qc_expand(mb, nb, Z, shifts, rp, ci);
      if (row_ptr_out_opt) std::copy(rp.begin(), rp.end(), row_ptr_out_opt);
      if (col_idx_out_opt) std::copy(ci.begin(), ci.end(), col_idx_out_opt);
    }
    // the block rows as a plan: mb layers of Z rows; nothing staged behind the frame
    ldpc::LayeredLayout lay;
    const bool fits = ldpc::layered_layout(mb * Z, nb * Z, entries * Z, row_max, mb, Z, precision, lay);
    if (lds_bytes_out_opt) *lds_bytes_out_opt = lay.frame;
    if (threads_out_opt) *threads_out_opt = lay.threads;
    return fits ? 1 : 0;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_decode_layered(ldpc_ctx *ctx, double scale, int max_iters, int et_period, int precision,
                        const float *in, int64_t n_in_floats, int64_t cw_stride, int elem_stride,
                        float polarity, int B, uint8_t *out_packed, uint8_t *out_bits_opt,
                        int32_t *iters_used_opt, int32_t *syn_weight_opt, float *llr_out_opt) {
  const ldpc::LayeredArith ar = float_arith(scale, precision);
  return decode_host_impl(ctx, LDPC_METHOD_LOGDOMAIN, max_iters, et_period, precision, in,
                          n_in_floats, cw_stride, elem_stride, polarity, B, false, out_packed,
                          out_bits_opt, iters_used_opt, syn_weight_opt, llr_out_opt, &ar);
}

int ldpc_decode_layered_device(ldpc_ctx *ctx, double scale, int max_iters, int et_period,
                               int precision, const float *d_in, int64_t cw_stride,
                               int elem_stride, float polarity, int B, uint8_t *d_out_packed,
                               uint8_t *d_out_bits_opt, int32_t *d_iters_used_opt,
                               int32_t *d_syn_weight_opt, float *d_llr_out_opt,
                               void *hip_stream) {
  return layered_device_impl(ctx, float_arith(scale, precision), max_iters, et_period, precision,
                             d_in, cw_stride, elem_stride, polarity, B, d_out_packed,
                             d_out_bits_opt, d_iters_used_opt, d_syn_weight_opt, d_llr_out_opt,
                             hip_stream);
}

// The rate-matched forms: the frame load recovers the context's pattern from
// the call's transmissions (ldpc_rate_match.hpp).  The plain decode's refusals
// come first, then the transmissions'.
int ldpc_decode_layered_rm(ldpc_ctx *ctx, double scale, int max_iters, int et_period,
                           int precision, const float *in, int64_t n_in_floats, int64_t rx_stride,
                           float polarity, int n_tx, const int32_t *k0, const int32_t *e,
                           float unreceived_lci, int B, uint8_t *out_packed,
                           uint8_t *out_bits_opt, int32_t *iters_used_opt,
                           int32_t *syn_weight_opt, float *llr_out_opt) {
  const ldpc::LayeredArith ar = float_arith(scale, precision);
  return rm_host(ctx, ar, max_iters, et_period, precision, in, n_in_floats, rx_stride, polarity,
                 n_tx, k0, e, unreceived_lci, B, out_packed, out_bits_opt, iters_used_opt,
                 syn_weight_opt, llr_out_opt);
}

int ldpc_decode_layered_rm_device(ldpc_ctx *ctx, double scale, int max_iters, int et_period,
                                  int precision, const float *d_in, int64_t rx_stride,
                                  float polarity, int n_tx, const int32_t *k0, const int32_t *e,
                                  float unreceived_lci, int B, uint8_t *d_out_packed,
                                  uint8_t *d_out_bits_opt, int32_t *d_iters_used_opt,
                                  int32_t *d_syn_weight_opt, float *d_llr_out_opt,
                                  void *hip_stream) {
  return rm_device(ctx, float_arith(scale, precision), max_iters, et_period, precision, d_in,
                   rx_stride, polarity, n_tx, k0, e, unreceived_lci, B, d_out_packed,
                   d_out_bits_opt, d_iters_used_opt, d_syn_weight_opt, d_llr_out_opt, hip_stream);
}

int ldpc_decode_layered_q8_rm(ldpc_ctx *ctx, int num, float llr_scale, int max_iters,
                              int et_period, const float *in, int64_t n_in_floats,
                              int64_t rx_stride, float polarity, int n_tx, const int32_t *k0,
                              const int32_t *e, float unreceived_lci, int B, uint8_t *out_packed,
                              uint8_t *out_bits_opt, int32_t *iters_used_opt,
                              int32_t *syn_weight_opt, float *llr_out_opt) {
  const ldpc::LayeredArith ar = q8_arith(num, llr_scale);
  return rm_host(ctx, ar, max_iters, et_period, LDPC_PREC_F32, in, n_in_floats, rx_stride,
                 polarity, n_tx, k0, e, unreceived_lci, B, out_packed, out_bits_opt,
                 iters_used_opt, syn_weight_opt, llr_out_opt);
}

int ldpc_decode_layered_q8_rm_device(ldpc_ctx *ctx, int num, float llr_scale, int max_iters,
                                     int et_period, const float *d_in, int64_t rx_stride,
                                     float polarity, int n_tx, const int32_t *k0,
                                     const int32_t *e, float unreceived_lci, int B,
                                     uint8_t *d_out_packed, uint8_t *d_out_bits_opt,
                                     int32_t *d_iters_used_opt, int32_t *d_syn_weight_opt,
                                     float *d_llr_out_opt, void *hip_stream) {
  return rm_device(ctx, q8_arith(num, llr_scale), max_iters, et_period, LDPC_PREC_F32, d_in,
                   rx_stride, polarity, n_tx, k0, e, unreceived_lci, B, d_out_packed,
                   d_out_bits_opt, d_iters_used_opt, d_syn_weight_opt, d_llr_out_opt, hip_stream);
}

// The code-block CRC of the layered decodes (ldpc_crc.hpp): the context's CRC
// and the remainders of its last decode.
int ldpc_set_crc(ldpc_ctx *ctx, int len, uint32_t poly, int mode) {
  if (!ctx) return LDPC_EINVAL;
  if (len == 0) {
    ctx->crc.len = 0;
    ctx->crc.last_B = 0;
    return LDPC_OK;
  }
  if (mode != LDPC_CRC_REPORT && mode != LDPC_CRC_STOP)
    return set_err(ctx, LDPC_EINVAL,
                   "mode must be LDPC_CRC_REPORT or LDPC_CRC_STOP (got " + std::to_string(mode) + ")");
  // a refused CRC leaves the one in force as it is
  const int rc = crc_upload(ctx, len, poly, ctx->rm.filler);
  if (rc != LDPC_OK) return rc;
  ctx->crc.mode = mode;
  ctx->crc.last_B = 0;
  return LDPC_OK;
}

int ldpc_crc_results(ldpc_ctx *ctx, uint32_t *out, int n) {
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Crc &c = ctx->crc;
  if (c.len == 0) return set_err(ctx, LDPC_EINVAL, "no CRC is set (ldpc_set_crc)");
  if (n < 0 || n > c.last_B || (n > 0 && !out))
    return set_err(ctx, LDPC_EINVAL,
                   "n must be in [0, " + std::to_string(c.last_B) +
                       "], the frames of the last layered decode (got " + std::to_string(n) + ")");
  if (n == 0) return LDPC_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  hipStream_t st = (hipStream_t)c.last_stream;
  if ((e = hipMemcpyAsync(out, c.d_rem, (size_t)n * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
    return hip_err(ctx, e, "hipMemcpyAsync(CRC results)");
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_err(ctx, e, "hipStreamSynchronize");
  return LDPC_OK;
}

const uint32_t *ldpc_crc_results_device(const ldpc_ctx *ctx) {
  return ctx && ctx->crc.len > 0 && ctx->crc.last_B > 0 ? ctx->crc.d_rem : nullptr;
}

int ldpc_plan_layers_q8(int M, int N, const int32_t *row_ptr, const int32_t *col_idx,
                        int32_t *layer_of_row_out_opt, int *n_layers_out_opt,
                        int64_t *lds_bytes_out_opt, int *threads_out_opt) {
  clear_create_error();
  if (!valid_csr(M, N, row_ptr, col_idx))
    return set_err(nullptr, LDPC_EINVAL, "CSR H must be M x N (M < N), columns ascending and in range");
  try {
    std::vector<int32_t> plan;
    const int L = ldpc::plan_layers(M, N, row_ptr, col_idx, plan);
    int dc_max = 0;
    for (int j = 0; j < M; ++j) dc_max = std::max(dc_max, row_ptr[j + 1] - row_ptr[j]);
    ldpc::LayeredLayout lay;
    const bool fits = ldpc::layered_q8_layout(M, N, row_ptr[M], dc_max,
                                              csr_dv_max(N, row_ptr[M], col_idx), L,
                                              largest_layer(plan, L), 0, lay);
    if (layer_of_row_out_opt) std::copy(plan.begin(), plan.end(), layer_of_row_out_opt);
    if (n_layers_out_opt) *n_layers_out_opt = L;
    if (lds_bytes_out_opt) *lds_bytes_out_opt = fits ? lay.total : lay.frame;
    if (threads_out_opt) *threads_out_opt = lay.threads;
    return fits ? 1 : 0;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_plan_qc_q8(int mb, int nb, int Z, const int32_t *shifts, int64_t *lds_bytes_out_opt,
                    int *threads_out_opt) {
  clear_create_error();
  std::string why;
  if (!ldpc::qc_check(mb, nb, Z, shifts, &why))
    return set_err(nullptr, LDPC_EINVAL, "bad quasi-cyclic code: " + why);
  int entries, row_max, col_max = 0;
  ldpc::qc_count(mb, nb, shifts, entries, row_max);
  for (int c = 0; c < nb; ++c) {
    int d = 0;
    for (int r = 0; r < mb; ++r) d += shifts[(size_t)r * nb + c] >= 0;
    col_max = std::max(col_max, d);
  }
  // the block rows as a plan: mb layers of Z rows; nothing staged behind the frame
  ldpc::LayeredLayout lay;
  const bool fits = ldpc::layered_q8_layout(mb * Z, nb * Z, (int64_t)entries * Z, row_max, col_max,
                                            mb, Z, Z, lay);
  if (lds_bytes_out_opt) *lds_bytes_out_opt = lay.frame;
  if (threads_out_opt) *threads_out_opt = lay.threads;
  return fits ? 1 : 0;
}

int ldpc_decode_layered_q8(ldpc_ctx *ctx, int num, float llr_scale, int max_iters, int et_period,
                           const float *in, int64_t n_in_floats, int64_t cw_stride,
                           int elem_stride, float polarity, int B, uint8_t *out_packed,
                           uint8_t *out_bits_opt, int32_t *iters_used_opt,
                           int32_t *syn_weight_opt, float *llr_out_opt) {
  const ldpc::LayeredArith ar = q8_arith(num, llr_scale);
  return decode_host_impl(ctx, LDPC_METHOD_LOGDOMAIN, max_iters, et_period, LDPC_PREC_F32, in,
                          n_in_floats, cw_stride, elem_stride, polarity, B, false, out_packed,
                          out_bits_opt, iters_used_opt, syn_weight_opt, llr_out_opt, &ar);
}

int ldpc_decode_layered_q8_device(ldpc_ctx *ctx, int num, float llr_scale, int max_iters,
                                  int et_period, const float *d_in, int64_t cw_stride,
                                  int elem_stride, float polarity, int B, uint8_t *d_out_packed,
                                  uint8_t *d_out_bits_opt, int32_t *d_iters_used_opt,
                                  int32_t *d_syn_weight_opt, float *d_llr_out_opt,
                                  void *hip_stream) {
  return layered_device_impl(ctx, q8_arith(num, llr_scale), max_iters, et_period, LDPC_PREC_F32,
                             d_in, cw_stride, elem_stride, polarity, B, d_out_packed,
                             d_out_bits_opt, d_iters_used_opt, d_syn_weight_opt, d_llr_out_opt,
                             hip_stream);
}

}  // extern "C"
