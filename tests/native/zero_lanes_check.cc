// Host check of the column-centric loop's forms in
// gr-ldpc_ece535a_amd/csrc/ldpc_exact.hpp: tanh_half_n's masked overload
// against the host libm and against the unmasked function, and the rewritten
// helpers (expm1_n's one-offset lookups, log_near1_lean) against the
// functions they replace.  Built by tests/test_exact_zero_lanes.py with
// -ffp-contract=off.  Every function returns the number of results whose bits
// differ (NaN == NaN) in out[0] and the largest ulp distance in out[1].
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../gr-ldpc_ece535a_amd/csrc/ldpc_exact.hpp"

using namespace ldpc::ex;

static const ExTab kEx = make_ex_tab();

static int64_t ulps(double a, double b) {
  if (a != a && b != b) return 0;
  if (bits(a) == bits(b)) return 0;
  int64_t ia = (int64_t)bits(a), ib = (int64_t)bits(b);
  if (ia < 0) ia = (int64_t)0x8000000000000000ull - ia;
  if (ib < 0) ib = (int64_t)0x8000000000000000ull - ib;
  const int64_t d = ia - ib;
  return d == 0 ? 1 : (d < 0 ? -d : d);  // +0 vs -0 counts as a mismatch
}

static void tally(double a, double b, int64_t *out) {
  const int64_t u = ulps(a, b);
  if (u) ++out[0];
  if (u > out[1]) out[1] = u;
}

// the host's mask is a per-value flag (LDPC_EX_LANES there).  mode 0: no flag
// set; 1: set exactly on the operands that are +-0; 2: set on none of the
// zeros (each takes the cold path) but on every operand inside the common
// range [2^-54, 13.5), where a set flag must change nothing
static uint64_t flag(int mode, double m) {
  if (mode == 1) return m == 0.0 ? 1 : 0;
  if (mode == 2) return fabs(m) >= 0x1p-54 && fabs(m) < 13.5 ? 1 : 0;
  return 0;
}

extern "C" {

// tanh_half_n<3>(m, zero) vs tanh(m / 2.0) (out[0..1]) and vs the unmasked
// tanh_half_n<3>(m) (out[2..3]), on consecutive triples (n % 3 == 0)
void check_tanh_masked(int mode, const double *m, int64_t n, int64_t *out) {
  out[0] = out[1] = out[2] = out[3] = 0;
  for (int64_t i = 0; i + 3 <= n; i += 3) {
    const double v[3] = {m[i], m[i + 1], m[i + 2]};
    const uint64_t zero[3] = {flag(mode, v[0]), flag(mode, v[1]), flag(mode, v[2])};
    double z[3], z0[3];
    tanh_half_n<3>(v, z, &kEx, zero);
    tanh_half_n<3>(v, z0, &kEx);
    for (int j = 0; j < 3; ++j) {
      tally(z[j], tanh(v[j] / 2.0), out);
      tally(z[j], z0[j], out + 2);
    }
  }
}

// expm1_n<3, true> vs expm1_n<3, false>: t and the k handed back
void check_expm1_lean(const double *u, int64_t n, int64_t *out) {
  out[0] = out[1] = 0;
  for (int64_t i = 0; i + 3 <= n; i += 3) {
    const double v[3] = {u[i], u[i + 1], u[i + 2]};
    uint32_t hx[3];
    for (int j = 0; j < 3; ++j) hx[j] = hiw(v[j]) & 0x7fffffffu;
    double t1[3], t0[3];
    int k1[3], k0[3];
    expm1_n<3, true>(v, hx, t1, k1, &kEx, true);
    expm1_n<3, false>(v, hx, t0, k0, &kEx, true);
    for (int j = 0; j < 3; ++j) {
      tally(t1[j], t0[j], out);
      if (k1[j] != k0[j]) ++out[0];
    }
  }
}

// log_near1_lean(x) vs log_near1(x)
void check_log_near1_lean(const double *x, int64_t n, int64_t *out) {
  out[0] = out[1] = 0;
  for (int64_t i = 0; i < n; ++i) tally(log_near1_lean(x[i]), log_near1(x[i]), out);
}

// fma3_(s, a, c) vs fma(s, a, c)
void check_fma3(const double *s, const double *a, const double *c, int64_t n, int64_t *out) {
  out[0] = out[1] = 0;
  for (int64_t i = 0; i < n; ++i) tally(fma3_(s[i], a[i], c[i]), fma(s[i], a[i], c[i]), out);
}
}
