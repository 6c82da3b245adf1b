// ldpc_probe.hip -- ldpc_math_probe (include/ldpc_hip.h): a test seam that
// evaluates the decode kernels' arithmetic (ldpc_device.hpp Math<PREC>,
// ldpc_exact.hpp, ldpc_math.hpp) operand by operand on the device, through
// the calls the kernels make, so that tests/test_gpu_math.py can hold each
// function to glibc with the device's own reciprocal seed and with 64
// unrelated operands per wave in every wave-uniform branch.
//
// One thread takes one group of three consecutive operands: one load, the
// call, one vector store.  Every lane of a launched wave stays active through
// the call (the wave-uniform regions ballot, and the packed log evaluates a
// packed cell on the lane of the same index); a thread past the last group
// computes on padding operands and stores nothing.  Built with the common
// HIPFLAGS (-ffp-contract=off), as the kernels are.
#include <hip/hip_runtime.h>

#include "ldpc_ctx.hpp"
#include "ldpc_device.hpp"

using namespace ldpc::capi;

namespace ldpc {
namespace {

constexpr int kProbeThreads = 256;
constexpr int kProbeWaves = kProbeThreads / 64;
// the packed log's LDS per wave: 64 lanes x 3 ratios, then the zero cell
// (ldpc_frame.hpp hands it tb and the cell at ebd)
constexpr int kPackCells = 64 * 3;

template <typename Real>
struct Pad {
  // a padding thread's operands: in every function's domain, on no cold path
  static __device__ __forceinline__ Real a(int fn) { return fn >= LDPC_PROBE_DIV1 ? Real(1) : Real(0.5); }
  static __device__ __forceinline__ Real b(int fn) { return fn >= LDPC_PROBE_DIV1 ? Real(1) : Real(0); }
};

template <int PREC, int FN>
__global__ void __launch_bounds__(kProbeThreads)
k_math_probe(const typename Math<PREC>::Real *a, const typename Math<PREC>::Real *b, int64_t groups,
             typename Math<PREC>::Real *out) {
  typedef typename Math<PREC>::Real Real;
  typedef typename Math<PREC>::Tab Tab;
  __shared__ Tab s_tab[TabLds<PREC>::kN];
  __shared__ double s_pack[kProbeWaves][kPackCells + 1];
  constexpr bool kPacked = FN == LDPC_PROBE_CHECK_MSG_PACKED || FN == LDPC_PROBE_CHECK_MSG_PACKED_LEAN;
  constexpr bool kTwo = FN == LDPC_PROBE_TANH_HALF_MASKED || FN >= LDPC_PROBE_DIV1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (kPacked && lane == 0) s_pack[wave][kPackCells] = 0.0;
  stage_tab<PREC>(s_tab);
  __syncthreads();
  const Tab *tab = s_tab;

  const int64_t g = (int64_t)blockIdx.x * kProbeThreads + threadIdx.x;
  const bool live = g < groups;
  Real x[3], y[3], z[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x[i] = live ? a[3 * g + i] : Pad<Real>::a(FN);
    y[i] = (kTwo && live) ? b[3 * g + i] : Pad<Real>::b(FN);
  }

  if constexpr (FN == LDPC_PROBE_TANH_HALF) {
    if constexpr (PREC == 0 || PREC == 2) {
      Math<PREC>::template tanh_half_n<3>(x, z, tab);
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = Math<PREC>::tanh_half(x[i], tab);
    }
  } else if constexpr (FN == LDPC_PROBE_TANH_HALF_MASKED) {
    uint64_t zero[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) zero[i] = __builtin_amdgcn_ballot_w64(y[i] != Real(0));
    Math<PREC>::template tanh_half_n<3>(x, z, tab, zero);
  } else if constexpr (FN == LDPC_PROBE_TANH_HALF_SMALL3) {
    fm::tanh_half_small_n<3>(x, z);
  } else if constexpr (FN == LDPC_PROBE_CHECK_MSG) {
    if constexpr (PREC == 0 || PREC == 2) {
      Math<PREC>::template check_msg_n<3>(x, tab, z);
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = Math<PREC>::check_msg(x[i], tab);
    }
  } else if constexpr (kPacked) {
    log_ratio_n_packed<3, FN == LDPC_PROBE_CHECK_MSG_PACKED_LEAN>(x, tab, z, s_pack[wave], lane,
                                                                  (uint32_t)kPackCells);
  } else if constexpr (FN == LDPC_PROBE_CHECK_MSG_OPEN3) {
    fm::log_ratio_tab_open_n<3>(x, tab, z);
  } else if constexpr (FN == LDPC_PROBE_DIV1) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double n1[1] = {x[i]}, d1[1] = {y[i]};
      double q1[1];
      ex::div_n<1>(n1, d1, q1);
      z[i] = q1[0];
    }
  } else if constexpr (FN == LDPC_PROBE_DIV2) {
    const double n0[2] = {x[0], x[1]}, d0[2] = {y[0], y[1]};
    const double n1[2] = {x[2], 1.0}, d1[2] = {y[2], 1.0};
    double q0[2], q1[2];
    ex::div_n<2>(n0, d0, q0);
    ex::div_n<2>(n1, d1, q1);
    z[0] = q0[0];
    z[1] = q0[1];
    z[2] = q1[0];
  } else {
    static_assert(FN == LDPC_PROBE_DIV3, "unknown probe function");
    if constexpr (PREC == 3)
      fm::div_fast_n<3>(x, y, z);
    else
      ex::div_n<3>(x, y, z);
  }

  if (live) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[3 * g + i] = z[i];
  }
}

template <int PREC, int FN>
int launch(const void *a, const void *b, int64_t groups, void *out, hipStream_t st) {
  typedef typename Math<PREC>::Real Real;
  const unsigned blocks = (unsigned)((groups + kProbeThreads - 1) / kProbeThreads);
  hipLaunchKernelGGL((k_math_probe<PREC, FN>), dim3(blocks), dim3(kProbeThreads), 0, st,
                     (const Real *)a, (const Real *)b, groups, (Real *)out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the (fn, precision) cells that exist; -2: no such cell.  groups == 0 only
// asks whether the cell exists (nothing is launched).
int dispatch(int fn, int prec, const void *a, const void *b, int64_t groups, void *out,
             hipStream_t st) {
#define LDPC_PROBE_CELL(F, P) \
  if (fn == (F) && prec == (P)) return groups > 0 ? launch<P, F>(a, b, groups, out, st) : 0
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF, 1);
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF, 2);
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF, 3);
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF_MASKED, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_TANH_HALF_SMALL3, 3);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG, 1);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG, 2);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG, 3);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG_PACKED, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG_PACKED_LEAN, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_CHECK_MSG_OPEN3, 3);
  LDPC_PROBE_CELL(LDPC_PROBE_DIV1, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_DIV2, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_DIV3, 0);
  LDPC_PROBE_CELL(LDPC_PROBE_DIV3, 3);
#undef LDPC_PROBE_CELL
  return -2;
}

}  // namespace
}  // namespace ldpc

extern "C" {

int ldpc_math_probe(ldpc_ctx *ctx, int fn, int precision, const void *d_a, const void *d_b_opt,
                    int64_t n, void *d_out) {
  serve_stop(ctx);
  if (!ctx) return LDPC_EINVAL;
  if (precision < 0 || precision > 3)
    return set_err(ctx, LDPC_EINVAL, "math probe: precision must be 0..3");
  if (fn < LDPC_PROBE_TANH_HALF || fn > LDPC_PROBE_DIV3)
    return set_err(ctx, LDPC_EINVAL, "math probe: unknown function " + std::to_string(fn));
  // mode 2 divides as mode 0 does (ex::div_n)
  const int cell_prec = (fn >= LDPC_PROBE_DIV1 && precision == LDPC_PREC_F64_LIBM) ? 0 : precision;
  const bool two = fn == LDPC_PROBE_TANH_HALF_MASKED || fn >= LDPC_PROBE_DIV1;
  // 2^31 - 1 blocks of 256 groups
  if (n < 0 || n % 3 != 0 || n / 3 > (int64_t)0x7fffffff * ldpc::kProbeThreads)
    return set_err(ctx, LDPC_EINVAL, "math probe: n must be a non-negative multiple of 3");
  if (n > 0 && (!d_a || !d_out || (two && !d_b_opt)))
    return set_err(ctx, LDPC_EINVAL, two ? "math probe: d_a, d_b_opt and d_out must be given"
                                         : "math probe: d_a and d_out must be given");
  hipError_t err = hipSetDevice(ctx->device);
  if (err != hipSuccess) return hip_err(ctx, err, "hipSetDevice");
  const int rc = ldpc::dispatch(fn, cell_prec, d_a, d_b_opt, n / 3, d_out, ctx->stream);
  if (rc == -2)
    return set_err(ctx, LDPC_EINVAL, "math probe: function " + std::to_string(fn) +
                                         " has no form at precision " + std::to_string(precision));
  return rc == 0 ? LDPC_OK : hip_err(ctx, hipGetLastError(), "math probe launch");
}

}  // extern "C"
