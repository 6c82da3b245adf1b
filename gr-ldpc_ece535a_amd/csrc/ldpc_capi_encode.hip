// ldpc_capi_encode.hip -- the C ABI of include/ldpc_hip.h: the device encoders
// of a context (ldpc_aux.hip: small, IRA staircase, quasi-cyclic), the
// quasi-cyclic encoder's host entry points, and the channel helpers
// (random bits, BPSK + AWGN, bit-error counts), and rate matching's device
// entry points (the context's pattern, the bit selector behind the encoder,
// the soft combiner in front of any decode).  Owns the context's encoder
// group (ldpc_ctx.hpp).
#include <stdio.h>

#include <exception>

#include "ldpc_aux.hpp"
#include "ldpc_ctx.hpp"
#include "ldpc_qc.hpp"
#include "ldpc_qc_enc.hpp"

using namespace ldpc::capi;

void ldpc_ctx::Encoder::release() {
  free_device(d_A);
  free_device(d_qc);
}

namespace {

// No device encoder for this context, now and on every later call.
int no_encoder(ldpc_ctx *ctx, const std::string &why) {
  ctx->encoder.kind = -1;
  ctx->encoder.err = why;
  return set_err(ctx, LDPC_EUNSUPPORTED, ctx->encoder.err);
}

// Systematic encoder of the context's H (codeword = [parity (M) | data (K)]):
// small codes get A = H_p^-1 H_d by Gauss-Jordan over GF(2) (unique when the
// first M columns are independent, which reorderHMatrix ensures); large codes
// must have the accumulator staircase in columns 0..M-1 (IRA / DVB-S2).  A
// quasi-cyclic context whose base matrix has an encodable parity part
// (ldpc_qc_enc.hpp) takes that encoder whatever its size -- the codeword is
// unique, so the small ones get the same bytes -- and any other falls through
// to the two rules above.
int prepare_encoder(ldpc_ctx *ctx) {
  const ldpc_ctx::Code &code = ctx->code;
  ldpc_ctx::Encoder &enc = ctx->encoder;
  if (enc.kind > 0) return LDPC_OK;
  if (enc.kind < 0) return set_err(ctx, LDPC_EUNSUPPORTED, enc.err);
  const int M = code.M, N = code.N, K = N - M;
  ldpc::QcEncProgram prog;
  if (code.qc_Z > 0 &&
      ldpc::qc_enc_compile(code.qc_mb, code.qc_nb, code.qc_Z, code.qc_shifts.data(), prog, nullptr)) {
    if (prog.lds_bytes() > ldpc::kQcEncLdsLimit) {
      char buf[200];
      snprintf(buf, sizeof buf,
               "quasi-cyclic encoder: the frame and its %d scratch blocks take %lld bytes of LDS "
               "(limit %lld): no device encoder",
               prog.scratch, (long long)prog.lds_bytes(), (long long)ldpc::kQcEncLdsLimit);
      return no_encoder(ctx, buf);
    }
    std::vector<uint32_t> tab;
    ldpc::qc_enc_pack(prog, tab);
    hipError_t e = hipMalloc(&enc.d_qc, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(enc.d_qc, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_err(ctx, e, "encoder upload");
    enc.qc_threads = prog.threads();
    enc.qc_lds = (int)prog.lds_bytes();
    enc.kind = 3;
    return LDPC_OK;
  }
  if (!code.H.empty() && K <= 256) {
    std::vector<uint64_t> A;
    if (!systematic_matrix(code.H.data(), M, N, A))
      return no_encoder(ctx, "the first M columns of H are dependent: no systematic encoder");
    hipError_t e = hipMalloc(&enc.d_A, A.size() * 8);
    if (e == hipSuccess) e = hipMemcpy(enc.d_A, A.data(), A.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_err(ctx, e, "encoder upload");
    enc.kind = 1;
    return LDPC_OK;
  }
  if (!has_staircase(M, code.rp.data(), code.ci.data()))
    return no_encoder(
        ctx, "large code without the accumulator staircase in columns 0..M-1: no device encoder");
  enc.kind = 2;
  return LDPC_OK;
}

}  // namespace

namespace ldpc {
namespace capi {

int rate_match_args(ldpc_ctx *ctx, int n_tx, const int32_t *k0, const int32_t *e,
                    float unreceived_lci, ldpc::RmArgs &rm, int64_t *total) {
  std::string why;
  if (!ldpc::rm_pattern(ctx->code.M, ctx->code.N, ctx->rm.punct, ctx->rm.filler, ctx->rm.ncb, rm,
                        &why))
    return set_err(ctx, LDPC_EINVAL, "bad rate-matching pattern: " + why);
  *total = ldpc::rm_transmissions(rm, n_tx, k0, e, &why);
  if (*total < 0) return set_err(ctx, LDPC_EINVAL, "bad transmission: " + why);
  if (unreceived_lci != unreceived_lci)
    return set_err(ctx, LDPC_EINVAL, "unreceived_lci must not be NaN");
  rm.unreceived = unreceived_lci;
  return LDPC_OK;
}

}  // namespace capi
}  // namespace ldpc

extern "C" {

int ldpc_set_rate_match(ldpc_ctx *ctx, int punct, int filler, int ncb) {
  if (!ctx) return LDPC_EINVAL;
  ldpc::RmArgs rm;
  std::string why;
  if (!ldpc::rm_pattern(ctx->code.M, ctx->code.N, punct, filler, ncb, rm, &why))
    return set_err(ctx, LDPC_EINVAL, "bad rate-matching pattern: " + why);
  // the CRC's block is what the fillers leave: it must stay longer than the
  // CRC, and its weights are those of the new length
  if (ctx->crc.len > 0) {
    const int rc = crc_upload(ctx, ctx->crc.len, ctx->crc.poly, filler);
    if (rc != LDPC_OK) return rc;
  }
  ctx->rm.punct = punct;
  ctx->rm.filler = filler;
  ctx->rm.ncb = ncb;
  return LDPC_OK;
}

int ldpc_crc_attach_device(ldpc_ctx *ctx, const uint8_t *d_payload, int B, uint8_t *d_info_out,
                           void *hip_stream) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Crc &c = ctx->crc;
  if (c.len == 0) return set_err(ctx, LDPC_EINVAL, "no CRC is set (ldpc_set_crc)");
  if (B < 0 || (B > 0 && (!d_payload || !d_info_out)))
    return set_err(ctx, LDPC_EINVAL, "bad arguments: B >= 0, buffers given");
  if (B == 0) return LDPC_OK;
  hipError_t err = hipSetDevice(ctx->device);
  if (err != hipSuccess) return hip_err(ctx, err, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  const int rc = ldpc::launch_crc_attach(c.d_w, c.len, c.A, ctx->code.N - ctx->code.M, d_payload, B,
                                         d_info_out, st);
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "crc_attach launch");
}

int ldpc_crc_check_device(ldpc_ctx *ctx, const uint8_t *d_packed, int B, uint32_t *d_rem_out,
                          void *hip_stream) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  const ldpc_ctx::Crc &c = ctx->crc;
  if (c.len == 0) return set_err(ctx, LDPC_EINVAL, "no CRC is set (ldpc_set_crc)");
  if (B < 0 || (B > 0 && (!d_packed || !d_rem_out)))
    return set_err(ctx, LDPC_EINVAL, "bad arguments: B >= 0, buffers given");
  if (B == 0) return LDPC_OK;
  hipError_t err = hipSetDevice(ctx->device);
  if (err != hipSuccess) return hip_err(ctx, err, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  const int rc = ldpc::launch_crc_check(c.d_w, c.A, ctx->code.KB, d_packed, B, d_rem_out, st);
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "crc_check launch");
}

int ldpc_rate_match_device(ldpc_ctx *ctx, const uint8_t *d_codewords, int B, int k0, int E,
                           uint8_t *d_out, int64_t out_stride, void *hip_stream) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  ldpc::RmArgs rm;
  int64_t total = 0;
  const int32_t k0s[1] = {k0}, es[1] = {E};
  int rc = rate_match_args(ctx, 1, k0s, es, 0.0f, rm, &total);
  if (rc != LDPC_OK) return rc;
  if (B < 0 || out_stride < E || (B > 0 && (!d_codewords || !d_out)))
    return set_err(ctx, LDPC_EINVAL, "bad arguments: B >= 0, out_stride >= E, buffers given");
  if (B == 0) return LDPC_OK;
  hipError_t err = hipSetDevice(ctx->device);
  if (err != hipSuccess) return hip_err(ctx, err, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  rc = ldpc::launch_rate_match(rm, d_codewords, B, d_out, out_stride, st);
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "rate_match launch");
}

int ldpc_rate_recover_device(ldpc_ctx *ctx, const float *d_rx, int64_t rx_stride, float polarity,
                             float unreceived_lci, int B, int n_tx, const int32_t *k0,
                             const int32_t *e, float *d_samples_out, void *hip_stream) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  ldpc::RmArgs rm;
  int64_t total = 0;
  int rc = rate_match_args(ctx, n_tx, k0, e, unreceived_lci, rm, &total);
  if (rc != LDPC_OK) return rc;
  if (B < 0 || rx_stride < total || (B > 0 && (!d_rx || !d_samples_out)))
    return set_err(ctx, LDPC_EINVAL,
                   "bad arguments: B >= 0, rx_stride >= the sum of E, buffers given");
  if (B == 0) return LDPC_OK;
  hipError_t err = hipSetDevice(ctx->device);
  if (err != hipSuccess) return hip_err(ctx, err, "hipSetDevice");
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  rc = ldpc::launch_rate_recover(rm, d_rx, rx_stride, polarity, B, d_samples_out, st);
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "rate_recover launch");
}

int ldpc_encode_device(ldpc_ctx *ctx, const uint8_t *d_data_bits, int B, uint8_t *d_codewords,
                       void *hip_stream) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  if (B < 0 || (B > 0 && (!d_data_bits || !d_codewords)))
    return set_err(ctx, LDPC_EINVAL, "bad encoder arguments");
  if (B == 0) return LDPC_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  int rc = prepare_encoder(ctx);
  if (rc != LDPC_OK) return rc;
  ldpc_ctx::Encoder &enc = ctx->encoder;
  void *st = hip_stream ? hip_stream : (void *)ctx->stream;
  const int M = ctx->code.M, K = ctx->code.N - M;
  if (enc.kind == 1)
    rc = ldpc::launch_encode_small(enc.d_A, M, K, d_data_bits, B, d_codewords, st);
  else if (enc.kind == 3)
    rc = ldpc::launch_encode_qc(enc.d_qc, ctx->code.qc_Z, M, K, enc.qc_threads, enc.qc_lds,
                                &enc.qc_lds_allowed, d_data_bits, B, d_codewords, st);
  else
    rc = ldpc::launch_encode_ira(ctx->graph.d_rp, ctx->graph.d_ci, M, K, d_data_bits, B,
                                 d_codewords, st);
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "encoder launch");
}

int ldpc_plan_qc_encoder(int mb, int nb, int Z, const int32_t *shifts, int *core_out_opt,
                         int *levels_out_opt, int64_t *lds_bytes_out_opt) {
  clear_create_error();
  std::string why;
  if (!ldpc::qc_check(mb, nb, Z, shifts, &why))
    return set_err(nullptr, LDPC_EINVAL, "bad quasi-cyclic code: " + why);
  try {
    ldpc::QcEncProgram prog;
    if (!ldpc::qc_enc_compile(mb, nb, Z, shifts, prog, &why)) {
      set_err(nullptr, LDPC_EUNSUPPORTED, "no quasi-cyclic encoder: " + why);
      return 0;
    }
    if (core_out_opt) *core_out_opt = prog.core;
    if (levels_out_opt) *levels_out_opt = prog.levels();
    if (lds_bytes_out_opt) *lds_bytes_out_opt = prog.lds_bytes();
    return 1;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_encode_qc(int mb, int nb, int Z, const int32_t *shifts, const uint8_t *data_bits, int B,
                   uint8_t *codewords_out) {
  clear_create_error();
  std::string why;
  if (!ldpc::qc_check(mb, nb, Z, shifts, &why))
    return set_err(nullptr, LDPC_EINVAL, "bad quasi-cyclic code: " + why);
  if (B < 0 || (B > 0 && (!data_bits || !codewords_out)))
    return set_err(nullptr, LDPC_EINVAL, "bad encoder arguments");
  try {
    ldpc::QcEncProgram prog;
    if (!ldpc::qc_enc_compile(mb, nb, Z, shifts, prog, &why))
      return set_err(nullptr, LDPC_EUNSUPPORTED, "no quasi-cyclic encoder: " + why);
    ldpc::qc_enc_run(prog, data_bits, B, codewords_out);
    return LDPC_OK;
  } catch (const std::exception &e) {
    return set_err(nullptr, LDPC_ENOMEM, e.what());
  }
}

int ldpc_random_bits(uint8_t *d_out, int64_t n, uint64_t seed, void *hip_stream) {
  if (n < 0 || (n > 0 && !d_out)) return set_err(nullptr, LDPC_EINVAL, "bad arguments");
  return ldpc::launch_random_bits(d_out, n, seed, hip_stream) == 0
             ? LDPC_OK
             : hip_err(nullptr, hipGetLastError(), "random_bits launch");
}

int ldpc_bpsk_awgn(const uint8_t *d_bits, int64_t n, float sigma, uint64_t seed, float *d_out,
                   void *hip_stream) {
  if (n < 0 || (n > 0 && (!d_bits || !d_out)) || !(sigma >= 0.0f))
    return set_err(nullptr, LDPC_EINVAL, "bad arguments");
  return ldpc::launch_bpsk_awgn(d_bits, n, sigma, seed, d_out, hip_stream) == 0
             ? LDPC_OK
             : hip_err(nullptr, hipGetLastError(), "bpsk_awgn launch");
}

int ldpc_count_bit_errors(const uint8_t *d_a, const uint8_t *d_b, int64_t per_frame, int B,
                          int32_t *d_counts, void *hip_stream) {
  if (B < 0 || per_frame < 0 || (B > 0 && (!d_a || !d_b || !d_counts)))
    return set_err(nullptr, LDPC_EINVAL, "bad arguments");
  return ldpc::launch_count_errors(d_a, d_b, per_frame, B, d_counts, hip_stream) == 0
             ? LDPC_OK
             : hip_err(nullptr, hipGetLastError(), "count_errors launch");
}

}  // extern "C"
