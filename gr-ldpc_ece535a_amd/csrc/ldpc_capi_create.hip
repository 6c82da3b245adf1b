// ldpc_capi_create.hip -- the C ABI of include/ldpc_hip.h (libldpc_hip.so):
// contexts.  The device edge tables of the decoder's H (small-code, large-code
// and on-chip), context creation and destruction, the queries and the knobs.
// Owns the context's code, small, graph (tables) and onchip groups
// (ldpc_ctx.hpp).  Every decode runs on the GPU; when no device is usable
// ldpc_create fails with LDPC_EDEVICE.
#include <stdio.h>

#include <exception>

#include "ldpc_ctx.hpp"
#include "ldpc_layout.hpp"
#include "ldpc_qc.hpp"

using namespace ldpc::capi;
using ldpc::ColRec;
using ldpc::EdgeColRec;
using ldpc::EdgeRowRec;
using ldpc::kNone;

namespace ldpc {
namespace capi {

int set_err(ldpc_ctx *ctx, int code, const std::string &msg) {
  if (!ctx) return set_create_error(code, msg);
  ctx->err = msg;
  return code;
}

int hip_err(ldpc_ctx *ctx, hipError_t e, const char *what) {
  return set_err(ctx, LDPC_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace capi
}  // namespace ldpc

void ldpc_ctx::Small::release() {
  free_device(d_erow);
  free_device(d_ecol);
  free_device(d_cols);
  free_device(d_rowmask);
  free_device(d_lane_col);
  free_device(d_col_lane);
}

void ldpc_ctx::Graph::release() {
  for (int32_t **p : {&d_rp, &d_ci, &d_cp, &d_ce, &d_cr}) free_device(*p);
  for (int32_t *&p : d_msn) free_device(p);
  for (ldpc::MsnDesc *&p : d_msnd) free_device(p);
  free_pinned(h_ctrl);
  if (d_work) {
    (void)hipDeviceSynchronize();  // graph decodes may run on caller streams
    free_device(d_work);
    work_bytes = 0;
  }
  if (done) (void)hipEventDestroy(done);
  done = nullptr;
  stream = nullptr;
}

void ldpc_ctx::Onchip::release() {
  for (uint32_t **p : {&d_erow, &d_ecol, &d_rows, &d_cols}) free_device(*p);
  free_device(d_ci);
  free_device(d_ce);
}

namespace {

// Edge / column / row tables of the decoder's H (see ldpc_kernels.hpp), at
// the cells and positions plan_layout chooses (search false: the plain CSR
// layout, LDPC_FLAG_PLAIN_LAYOUT).
int build_tables(ldpc_ctx *ctx, std::vector<EdgeRowRec> &erecs, std::vector<EdgeColRec> &crecs,
                 std::vector<ColRec> &cols, std::vector<uint64_t> &rowmask,
                 std::vector<uint16_t> &lane_col, std::vector<uint8_t> &col_lane,
                 bool search, std::vector<int> *cell_out = nullptr) {
  ldpc_ctx::Code &code = ctx->code;
  const int M = code.M, N = code.N;
  const uint8_t *H = code.H.data();
  std::vector<std::vector<int>> row_edges(M), col_edges(N);
  std::vector<int> erow, ecol;
  for (int j = 0; j < M; ++j)
    for (int i = 0; i < N; ++i)
      if (H[(size_t)j * N + i]) {
        const int e = (int)erow.size();
        erow.push_back(j);
        ecol.push_back(i);
        row_edges[j].push_back(e);
        col_edges[i].push_back(e);  // rows ascend because j ascends
      }
  code.E = (int)erow.size();
  code.dc_max = 0;
  code.dv_max = 0;
  for (auto &r : row_edges) code.dc_max = std::max(code.dc_max, (int)r.size());
  code.dc_min = code.dc_max;
  for (auto &r : row_edges) code.dc_min = std::min(code.dc_min, (int)r.size());
  for (auto &c : col_edges) code.dv_max = std::max(code.dv_max, (int)c.size());
  if (code.E == 0) return set_err(ctx, LDPC_EINVAL, "H has no ones");
  if (N > ldpc::kNMax || M > ldpc::kMMax || code.E > 64 * ldpc::kSlotsMax ||
      code.dc_max > ldpc::kDcMax || code.dv_max > ldpc::kDvMax) {
    char buf[256];
    snprintf(buf, sizeof buf,
             "code shape outside the small-code kernel (M=%d N=%d E=%d dc_max=%d dv_max=%d; "
             "limits M,N<=%d E<=%d dc<=%d dv<=%d)",
             M, N, code.E, code.dc_max, code.dv_max, ldpc::kNMax, 64 * ldpc::kSlotsMax,
             ldpc::kDcMax, ldpc::kDvMax);
    return set_err(ctx, LDPC_EUNSUPPORTED, buf);
  }
  ctx->slots = (code.E + 63) / 64;
  ctx->nw = N <= 64 ? 1 : 4;
  ctx->rs = (M + 63) / 64;
  const int slots = ctx->slots, nw = ctx->nw;
  code.K = N - M;
  code.KB = (code.K + 7) / 8;

  // the loop lengths the small-code kernels are instantiated with for this
  // code, and whether sum-product runs its column-centric form: the one
  // shape rule (ldpc_kernels.hpp) the launchers dispatch by
  const ldpc::KernelShape shape = ldpc::kernel_shape(nw, slots, code.dc_max, code.dv_max);
  const ldpc::EdgeLayout lay = ldpc::plan_layout(M, N, erow, ecol, slots, nw, shape.dcn, shape.dvn,
                                                 shape.cols, search);
  const std::vector<int> &cell = lay.slot, &pos = lay.pos;
  if (cell_out) *cell_out = cell;
  int *model = ctx->small.layout_model;
  model[0] = lay.searched ? 1 : 0;
  model[1] = lay.model_cc;
  model[2] = lay.model_ec;
  model[3] = lay.plain_cc;
  model[4] = lay.plain_ec;
  uint64_t *dpos = ctx->small.dpos;
  dpos[0] = dpos[1] = 0;
  for (int g = 0; g < 2 * slots; ++g) dpos[g / 8] |= (uint64_t)(lay.dpos[g] & 31) << (8 * (g % 8));

  erecs.assign((size_t)64 * slots, EdgeRowRec{});
  crecs.assign((size_t)64 * slots, EdgeColRec{});
  for (auto &r : erecs) {
    std::fill(std::begin(r.rn), std::end(r.rn), kNone);
    r.col = kNone;
  }
  for (auto &r : crecs) {
    std::fill(std::begin(r.cn), std::end(r.cn), kNone);
    r.col = kNone;
  }
  for (int e = 0; e < code.E; ++e) {
    EdgeRowRec &er = erecs[cell[e]];
    EdgeColRec &ec = crecs[cell[e]];
    er.col = ec.col = (uint16_t)pos[ecol[e]];
    int k = 0;
    for (int n : row_edges[erow[e]])
      if (n != e) er.rn[k++] = (uint16_t)cell[n];  // ascending column
    k = 0;
    for (int n : col_edges[ecol[e]])
      if (n != e) ec.cn[k++] = (uint16_t)cell[n];  // ascending row
  }
  cols.assign((size_t)64 * nw, ColRec{});
  for (auto &c : cols) {
    std::fill(std::begin(c.e), std::end(c.e), kNone);
    std::fill(std::begin(c.r), std::end(c.r), kNone);
  }
  lane_col.assign((size_t)64 * nw, kNone);
  col_lane.assign((size_t)N, 0);
  for (int i = 0; i < N; ++i) {
    lane_col[pos[i]] = (uint16_t)i;
    col_lane[i] = (uint8_t)pos[i];
    for (size_t k = 0; k < col_edges[i].size(); ++k) {
      cols[pos[i]].e[k] = (uint16_t)cell[col_edges[i][k]];
      cols[pos[i]].r[k] = (uint16_t)erow[col_edges[i][k]];
    }
  }
  rowmask.assign((size_t)M * nw, 0);
  for (int j = 0; j < M; ++j)
    for (int i = 0; i < N; ++i)
      if (H[(size_t)j * N + i]) rowmask[(size_t)j * nw + pos[i] / 64] |= 1ull << (pos[i] % 64);
  // behind the row masks, the static zero lanes of the column-centric
  // sum-product (CodeView::rowmask): word q * kDvMax + k has bit l set when
  // entry k of position l + 64 q is the only entry its column can have --
  // every other entry of the record is missing (a column of degree 1 gives
  // its entry 0, a column of degree 0 or a position past N all of them).
  // That entry's bit message, the sum over the column's other entries, is then
  // the empty sum +0.0 in every iteration of every all-finite frame.
  rowmask.resize((size_t)M * nw + (size_t)nw * ldpc::kDvMax, 0);
  for (int p = 0; p < 64 * nw; ++p)
    for (int k = 0; k < ldpc::kDvMax; ++k) {
      bool alone = true;
      for (int k2 = 0; k2 < ldpc::kDvMax; ++k2) alone = alone && (k2 == k || cols[p].e[k2] == kNone);
      if (alone) rowmask[(size_t)M * nw + (size_t)(p / 64) * ldpc::kDvMax + k] |= 1ull << (p % 64);
    }
  return LDPC_OK;
}

// Degrees and the CSC permutation of the context's CSR; checks the
// large-code kernels' degree limits.
int build_graph(ldpc_ctx *ctx, std::vector<int32_t> &cp, std::vector<int32_t> &ce,
                std::vector<int32_t> &cr) {
  ldpc_ctx::Code &code = ctx->code;
  const int M = code.M, N = code.N;
  code.E = code.rp[M];
  if (code.E == 0) return set_err(ctx, LDPC_EINVAL, "H has no ones");
  cp.assign((size_t)N + 1, 0);
  for (int e = 0; e < code.E; ++e) cp[code.ci[e] + 1]++;
  code.dc_max = 0;
  code.dv_max = 0;
  for (int i = 0; i < N; ++i) code.dv_max = std::max(code.dv_max, cp[i + 1]);
  for (int j = 0; j < M; ++j) code.dc_max = std::max(code.dc_max, code.rp[j + 1] - code.rp[j]);
  for (int i = 0; i < N; ++i) cp[i + 1] += cp[i];
  ce.assign((size_t)code.E, 0);
  cr.assign((size_t)code.E, 0);
  std::vector<int32_t> fill(cp.begin(), cp.end() - 1);
  for (int j = 0; j < M; ++j)
    for (int32_t e = code.rp[j]; e < code.rp[j + 1]; ++e) {
      const int32_t k = fill[code.ci[e]]++;  // rows ascend because j ascends
      ce[k] = e;
      cr[k] = j;
    }
  if (code.dc_max > ldpc::kGraphDcMax || code.dv_max > ldpc::kGraphDvMax) {
    char buf[160];
    snprintf(buf, sizeof buf,
             "code degrees outside the large-code kernels (dc_max=%d dv_max=%d; limits %d, %d)",
             code.dc_max, code.dv_max, ldpc::kGraphDcMax, ldpc::kGraphDvMax);
    return set_err(ctx, LDPC_EUNSUPPORTED, buf);
  }
  code.K = N - M;
  code.KB = (code.K + 7) / 8;
  ctx->graph.on = true;
  return LDPC_OK;
}

// LDPC_FLAG_ONCHIP: the code must fit the on-chip kernels for both methods at
// every precision (ldpc_plan_onchip); decided from the shape alone, before
// any device is looked up.
int check_onchip(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  for (int method = 0; method < 2; ++method)
    for (int prec = 0; prec < 4; ++prec) {
      ldpc::OnchipLayout L;
      if (ldpc::onchip_plan(code.M, code.N, code.E, code.dc_max, code.dv_max, method, prec, L))
        continue;
      char buf[256];
      if (L.frame > ldpc::kOnchipLdsLimit)
        snprintf(buf, sizeof buf,
                 "the code does not fit the on-chip kernels: a frame needs %d bytes of LDS "
                 "(method %d, precision %d), the limit is %d (M=%d N=%d E=%d)",
                 L.frame, method, prec, ldpc::kOnchipLdsLimit, code.M, code.N, code.E);
      else
        snprintf(buf, sizeof buf,
                 "the code does not fit the on-chip kernels: M, N, E must be <= %d (M=%d N=%d "
                 "E=%d; a frame needs %d bytes of LDS, the limit is %d)",
                 ldpc::kOnchipIndexMax, code.M, code.N, code.E, L.frame, ldpc::kOnchipLdsLimit);
      return set_err(ctx, LDPC_EUNSUPPORTED, buf);
    }
  return LDPC_OK;
}

// Device setup shared by ldpc_create / ldpc_create_csr: the context's H is
// in code.rp / code.ci (and code.H for small codes).  Picks the small-code
// kernel when the code fits it (unless LDPC_FLAG_GRAPH), else the large-code
// path.  Consumes ctx on failure.
ldpc_ctx *finish_create(ldpc_ctx *ctx, int flags, int device) {
  std::vector<EdgeRowRec> erecs;
  std::vector<EdgeColRec> crecs;
  std::vector<ColRec> cols;
  std::vector<uint64_t> rowmask;
  std::vector<uint16_t> lane_col;
  std::vector<uint8_t> col_lane;
  std::vector<int32_t> cp, ce, cr;
  ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Graph &graph = ctx->graph;
  const auto refuse = [&](const std::string &msg) -> ldpc_ctx * {
    set_err(nullptr, LDPC_EINVAL, msg);
    delete ctx;
    return nullptr;
  };
  const bool onchip = (flags & LDPC_FLAG_ONCHIP) != 0;
  if (onchip && (flags & LDPC_FLAG_GRAPH))
    return refuse("LDPC_FLAG_ONCHIP and LDPC_FLAG_GRAPH exclude each other");
  ldpc::OnchipTables oct;
  int rc = LDPC_EUNSUPPORTED;
  if (!(flags & (LDPC_FLAG_GRAPH | LDPC_FLAG_ONCHIP)) && !code.H.empty())
    rc = build_tables(ctx, erecs, crecs, cols, rowmask, lane_col, col_lane,
                      !(flags & LDPC_FLAG_PLAIN_LAYOUT));
  if (rc == LDPC_EUNSUPPORTED) {
    ctx->err.clear();
    rc = build_graph(ctx, cp, ce, cr);
  }
  if (rc == LDPC_OK && onchip) {
    rc = check_onchip(ctx);
    if (rc == LDPC_OK) {
      ctx->onchip.on = true;
      ldpc::onchip_build(code.M, code.N, code.rp, code.ci, cp, ce, oct);
    }
  }
  if (rc != LDPC_OK) return refuse(ctx->err);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
    return refuse(std::string("no usable HIP device (") +
                  (e != hipSuccess ? hipGetErrorString(e) : "device index out of range") +
                  "); the decode path has no CPU fallback");
  ctx->device = device;
  // large-code min-sum: the narrow-chunk pipeline's tables
  graph.narrow = graph.on && !ctx->onchip.on && code.M <= ldpc::kMsnMaxRows;
  if (graph.narrow) {
    try {
      ldpc::msn_build(code.M, code.N, code.rp, code.ci, graph.msn);
    } catch (const std::exception &ex) {
      return refuse(ex.what());
    }
  }
  const char *what = nullptr;
  if ((e = hipSetDevice(device)) != hipSuccess) what = "hipSetDevice";
  if (!what && (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess)
    what = "hipStreamCreate";
  if (graph.on) {
    upload(&graph.d_rp, code.rp, "upload(row_ptr)", what, e);
    upload(&graph.d_ci, code.ci, "upload(col_idx)", what, e);
    upload(&graph.d_cp, cp, "upload(col_ptr)", what, e);
    upload(&graph.d_ce, ce, "upload(col_edges)", what, e);
    upload(&graph.d_cr, cr, "upload(col_rows)", what, e);
    if (graph.narrow) {
      const std::vector<int32_t> *t[4] = {&graph.msn.rx, &graph.msn.cx, &graph.msn.corig,
                                          &graph.msn.cpos};
      for (int i = 0; i < 4; ++i) upload(&graph.d_msn[i], *t[i], "upload(storage order)", what, e);
      upload(&graph.d_msnd[0], graph.msn.rdesc, "upload(edge descriptors)", what, e);
      upload(&graph.d_msnd[1], graph.msn.cdesc, "upload(edge descriptors)", what, e);
    }
    if (ctx->onchip.on) {
      ldpc_ctx::Onchip &oc = ctx->onchip;
      upload(&oc.d_erow, oct.erow, "upload(on-chip rows of edges)", what, e);
      upload(&oc.d_ecol, oct.ecol, "upload(on-chip columns of edges)", what, e);
      upload(&oc.d_rows, oct.rows, "upload(on-chip rows)", what, e);
      upload(&oc.d_cols, oct.cols, "upload(on-chip columns)", what, e);
      upload(&oc.d_ci, oct.ci, "upload(on-chip col_idx)", what, e);
      upload(&oc.d_ce, oct.ce, "upload(on-chip col_edges)", what, e);
      ensure_tickets(ctx, what, e);
    }
  } else {
    ldpc_ctx::Small &s = ctx->small;
    upload(&s.d_erow, erecs, "upload(erow)", what, e);
    upload(&s.d_ecol, crecs, "upload(ecol)", what, e);
    upload(&s.d_cols, cols, "upload(cols)", what, e);
    upload(&s.d_rowmask, rowmask, "upload(rowmask)", what, e);
    upload(&s.d_lane_col, lane_col, "upload(lane_col)", what, e);
    upload(&s.d_col_lane, col_lane, "upload(col_lane)", what, e);
    ensure_tickets(ctx, what, e);
  }
  if (what) {
    set_err(nullptr, LDPC_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
    ldpc_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

// ldpc_create_csr and ldpc_create_qc (qc: the base matrix the CSR was expanded
// from, which the context remembers): the same context either way.
struct QcSpec {
  int mb, nb, Z;
  const int32_t *shifts;
};

ldpc_ctx *create_from_csr(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int flags,
                          const QcSpec *qc, int device) {
  if (!valid_csr(M, N, row_ptr, col_idx)) {
    set_err(nullptr, LDPC_EINVAL,
            "CSR H must be M x N (M < N), row_ptr[0] == 0, non-decreasing, columns ascending "
            "and in range");
    return nullptr;
  }
  ldpc_ctx *ctx = new ldpc_ctx();
  ldpc_ctx::Code &code = ctx->code;
  code.M = M;
  code.N = N;
  code.rp.assign(row_ptr, row_ptr + M + 1);
  code.ci.assign(col_idx, col_idx + row_ptr[M]);
  if (N <= ldpc::kNMax && M <= ldpc::kMMax) {  // small enough for the register kernel
    code.H.assign((size_t)M * N, 0);
    for (int j = 0; j < M; ++j)
      for (int32_t e = row_ptr[j]; e < row_ptr[j + 1]; ++e) code.H[(size_t)j * N + col_idx[e]] = 1;
  }
  if (qc) {
    code.qc_mb = qc->mb;
    code.qc_nb = qc->nb;
    code.qc_Z = qc->Z;
    code.qc_shifts.assign(qc->shifts, qc->shifts + (size_t)qc->mb * qc->nb);
    ctx->layered.qc_tables = (flags & LDPC_FLAG_QC_TABLES) != 0;
  }
  return finish_create(ctx, flags, device);
}

// ldpc_create and ldpc_create_csr take no LDPC_FLAG_QC_TABLES.
bool refuse_qc_tables(int flags) {
  if (!(flags & LDPC_FLAG_QC_TABLES)) return false;
  set_err(nullptr, LDPC_EINVAL, "LDPC_FLAG_QC_TABLES belongs to ldpc_create_qc");
  return true;
}

}  // namespace

extern "C" {

ldpc_ctx *ldpc_create(const uint8_t *H, int M, int N, int flags, int device) {
  clear_create_error();
  if (refuse_qc_tables(flags)) return nullptr;
  if (!valid_h(H, M, N)) {
    set_err(nullptr, LDPC_EINVAL, "H must be M x N (M < N) with 0/1 entries");
    return nullptr;
  }
  ldpc_ctx *ctx = new ldpc_ctx();
  ldpc_ctx::Code &code = ctx->code;
  code.M = M;
  code.N = N;
  code.H.assign(H, H + (size_t)M * N);
  if (!(flags & LDPC_FLAG_NO_REORDER)) reorder_columns(code.H.data(), M, N, nullptr, nullptr, nullptr);
  dense_to_csr(code.H.data(), M, N, code.rp, code.ci);
  return finish_create(ctx, flags, device);
}

ldpc_ctx *ldpc_create_csr(int M, int N, const int32_t *row_ptr, const int32_t *col_idx,
                          int flags, int device) {
  clear_create_error();
  if (refuse_qc_tables(flags)) return nullptr;
  return create_from_csr(M, N, row_ptr, col_idx, flags, nullptr, device);
}

ldpc_ctx *ldpc_create_qc(int mb, int nb, int Z, const int32_t *shifts, int flags, int device) {
  clear_create_error();
  std::string why;
  if (!ldpc::qc_check(mb, nb, Z, shifts, &why)) {
    set_err(nullptr, LDPC_EINVAL, "bad quasi-cyclic code: " + why);
    return nullptr;
  }
  try {
    const QcSpec qc{mb, nb, Z, shifts};
    std::vector<int32_t> rp, ci;
    ldpc::qc_expand(mb, nb, Z, shifts, rp, ci);
    return create_from_csr(mb * Z, nb * Z, rp.data(), ci.data(), flags, &qc, device);
  } catch (const std::exception &e) {
    set_err(nullptr, LDPC_ENOMEM, e.what());
    return nullptr;
  }
}

// Also runs on a half-built context (finish_create).  The order is that of
// the synchronisations: the sessions end first, the ring's stream is waited
// for before it goes, the context's stream before the tables, the device
// before the large-code workspace; the context's stream goes last.
void ldpc_destroy(ldpc_ctx *ctx) {
  if (!ctx) return;
  serve_stop(ctx);
  if (ctx->ring.on) (void)ldpc_ring_end(ctx);
  ctx->ring.release();
  const ldpc_ctx::Stage &st = ctx->stage;
  if (st.profile && st.calls)
    fprintf(stderr,
            "ldpc_decode_windows profile: %lld calls, %lld windows; staging %.3f ms, window list + "
            "launch %.3f ms, wait %.3f ms, results %.3f ms\n",
            st.calls, st.windows, 1e3 * st.prof[0], 1e3 * st.prof[1], 1e3 * st.prof[2],
            1e3 * st.prof[3]);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  ctx->small.release();
  ctx->stage.release();
  ctx->serve.release();
  ctx->queues.release();
  ctx->onchip.release();
  ctx->layered.release();
  ctx->crc.release();
  ctx->graph.release();
  ctx->encoder.release();
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *ldpc_last_error(const ldpc_ctx *ctx) {
  return ctx ? ctx->err.c_str() : create_error().c_str();
}

int ldpc_ctx_info(const ldpc_ctx *ctx, int *M, int *N, int *E, int *K, int *KB, int *dc_max,
                  int *dv_max) {
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Code &code = ctx->code;
  if (M) *M = code.M;
  if (N) *N = code.N;
  if (E) *E = code.E;
  if (K) *K = code.K;
  if (KB) *KB = code.KB;
  if (dc_max) *dc_max = code.dc_max;
  if (dv_max) *dv_max = code.dv_max;
  return LDPC_OK;
}

int ldpc_ctx_h(const ldpc_ctx *ctx, uint8_t *H_out) {
  if (!ctx || !H_out) return LDPC_EINVAL;
  const ldpc_ctx::Code &code = ctx->code;
  memset(H_out, 0, (size_t)code.M * code.N);
  for (int j = 0; j < code.M; ++j)
    for (int32_t e = code.rp[j]; e < code.rp[j + 1]; ++e) H_out[(size_t)j * code.N + code.ci[e]] = 1;
  return LDPC_OK;
}

int ldpc_ctx_csr(const ldpc_ctx *ctx, int32_t *row_ptr_out, int32_t *col_idx_out) {
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Code &code = ctx->code;
  if (row_ptr_out) memcpy(row_ptr_out, code.rp.data(), code.rp.size() * sizeof(int32_t));
  if (col_idx_out) memcpy(col_idx_out, code.ci.data(), code.ci.size() * sizeof(int32_t));
  return LDPC_OK;
}

int ldpc_ctx_path(const ldpc_ctx *ctx) {
  if (!ctx) return LDPC_EINVAL;
  return ctx->onchip.on ? 2 : ctx->graph.on ? 1 : 0;
}

int ldpc_ctx_pipeline(const ldpc_ctx *ctx, int *frames_per_chunk, int *chunks) {
  if (!ctx) return LDPC_EINVAL;
  const bool narrow = ctx->graph.narrow;
  if (frames_per_chunk) *frames_per_chunk = narrow ? ldpc::kMsnFrames : 0;
  if (chunks) *chunks = narrow ? ldpc::msn_default_chunks() : 0;
  return narrow ? 1 : 0;
}

int ldpc_ctx_layout(const ldpc_ctx *ctx, int32_t *model_out) {
  if (!ctx || !model_out) return LDPC_EINVAL;
  if (ctx->graph.on) return LDPC_EUNSUPPORTED;
  std::copy(ctx->small.layout_model, ctx->small.layout_model + 5, model_out);
  return LDPC_OK;
}

int ldpc_ctx_qc(const ldpc_ctx *ctx, int *mb, int *nb, int *Z, int32_t *shifts_out_opt) {
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Code &code = ctx->code;
  if (mb) *mb = code.qc_mb;
  if (nb) *nb = code.qc_nb;
  if (Z) *Z = code.qc_Z;
  if (code.qc_Z <= 0) return 0;
  if (shifts_out_opt) std::copy(code.qc_shifts.begin(), code.qc_shifts.end(), shifts_out_opt);
  return 1;
}

int ldpc_plan_storage_order(int M, int N, const int32_t *row_ptr, const int32_t *col_idx,
                            int32_t *rpos_out_opt, int32_t *cpos_out_opt, int64_t *score_out_opt) {
  clear_create_error();
  if (!valid_csr(M, N, row_ptr, col_idx))
    return set_err(nullptr, LDPC_EINVAL, "CSR H must be M x N (M < N), columns ascending and in range");
  try {
    std::vector<int32_t> rp(row_ptr, row_ptr + M + 1), ci(col_idx, col_idx + row_ptr[M]);
    ldpc::MsnTables t;
    ldpc::msn_build(M, N, rp, ci, t);
    if (rpos_out_opt) std::copy(t.rpos.begin(), t.rpos.end(), rpos_out_opt);
    if (cpos_out_opt) std::copy(t.cpos.begin(), t.cpos.end(), cpos_out_opt);
    if (score_out_opt) {
      score_out_opt[0] = t.score[0];
      score_out_opt[1] = t.score[1];
    }
    return t.order;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_plan_layout(const uint8_t *H, int M, int N, int flags, int32_t *cell_out_opt,
                     int32_t *pos_out_opt, int32_t *model_out_opt) {
  clear_create_error();
  if (!valid_h(H, M, N)) return set_err(nullptr, LDPC_EINVAL, "H must be M x N (M < N) with 0/1 entries");
  ldpc_ctx tmp;
  tmp.code.M = M;
  tmp.code.N = N;
  tmp.code.H.assign(H, H + (size_t)M * N);
  if (!(flags & LDPC_FLAG_NO_REORDER))
    reorder_columns(tmp.code.H.data(), M, N, nullptr, nullptr, nullptr);
  std::vector<EdgeRowRec> erecs;
  std::vector<EdgeColRec> crecs;
  std::vector<ColRec> cols;
  std::vector<uint64_t> rowmask;
  std::vector<uint16_t> lane_col;
  std::vector<uint8_t> col_lane;
  std::vector<int> cell;
  const int rc = build_tables(&tmp, erecs, crecs, cols, rowmask, lane_col, col_lane,
                              !(flags & LDPC_FLAG_PLAIN_LAYOUT), &cell);
  if (rc != LDPC_OK) return set_err(nullptr, rc, tmp.err);
  if (cell_out_opt) std::copy(cell.begin(), cell.end(), cell_out_opt);
  if (pos_out_opt)
    for (int i = 0; i < N; ++i) pos_out_opt[i] = col_lane[i];
  if (model_out_opt) std::copy(tmp.small.layout_model, tmp.small.layout_model + 5, model_out_opt);
  return tmp.code.E;
}

int ldpc_plan_onchip(int M, int N, int E, int dc_max, int dv_max, int method, int precision,
                     int64_t *lds_bytes_out_opt, int *threads_out_opt) {
  clear_create_error();
  if (M <= 0 || N <= 0 || M >= N || E <= 0 || dc_max < 1 || dv_max < 1)
    return set_err(nullptr, LDPC_EINVAL, "M, N (M < N), E and the degrees must be positive");
  if (method != LDPC_METHOD_LOGDOMAIN && method != LDPC_METHOD_SUMPRODUCT)
    return set_err(nullptr, LDPC_EINVAL, "the on-chip kernels take min-sum and sum-product");
  if (precision < 0 || precision > 3)
    return set_err(nullptr, LDPC_EINVAL, "precision must be one of LDPC_PREC_*");
  ldpc::OnchipLayout L;
  const bool fits = ldpc::onchip_plan(M, N, E, dc_max, dv_max, method, precision, L);
  if (lds_bytes_out_opt) *lds_bytes_out_opt = fits ? L.total : L.frame;
  if (threads_out_opt) *threads_out_opt = L.threads;
  return fits ? 1 : 0;
}

int ldpc_set_work_limit(ldpc_ctx *ctx, int64_t bytes) {
  if (!ctx || bytes < 0) return set_err(ctx, LDPC_EINVAL, "work limit must be >= 0");
  ctx->graph.work_limit = bytes ? (size_t)bytes : ((size_t)8 << 30);
  return LDPC_OK;
}

int ldpc_set_waves_per_cu(ldpc_ctx *ctx, int waves_per_cu) {
  if (!ctx || waves_per_cu < 0 || waves_per_cu > 32)
    return set_err(ctx, LDPC_EINVAL, "waves_per_cu must be in [0, 32]");
  ctx->small.waves_per_cu = waves_per_cu;
  return LDPC_OK;
}

int ldpc_set_launch_mode(ldpc_ctx *ctx, int mode) {
  if (!ctx || (mode != LDPC_MODE_LATENCY && mode != LDPC_MODE_THROUGHPUT))
    return set_err(ctx, LDPC_EINVAL, "mode must be LDPC_MODE_LATENCY or LDPC_MODE_THROUGHPUT");
  // measured on the config-2 batch (profiles/round2/ab_launch_mode.txt,
  // profiles/round2/layout/): one launch at a time: 12 waves per CU, priority
  // for starved waves; overlapping launches: 4 waves per CU each (4 launches
  // in flight fill the CU's 16 wave slots of the throughput build), no
  // priority games
  ctx->small.waves_per_cu = mode == LDPC_MODE_THROUGHPUT ? 4 : 0;
  ctx->small.fair_cycles = mode == LDPC_MODE_THROUGHPUT ? 0 : 1800;
  return LDPC_OK;
}

int ldpc_set_schedule(ldpc_ctx *ctx, int schedule) {
  if (!ctx || schedule < 0 || schedule > 2)
    return set_err(ctx, LDPC_EINVAL, "schedule must be 0 (auto), 1 or 2");
  ctx->small.schedule = schedule;
  return LDPC_OK;
}

int ldpc_synchronize(ldpc_ctx *ctx) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  hipError_t e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? LDPC_OK : hip_err(ctx, e, "hipStreamSynchronize");
}

}  // extern "C"
