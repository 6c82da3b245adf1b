// Host check of div_n's reciprocals (gr-ldpc_ece535a_amd/csrc/ldpc_exact.hpp):
// every yk that div_recips hands to div_core must put b * yk inside
// (1 + 2^-41, 1 + 2^-39), and every quotient must equal the host's a / b.
// Built by tests/test_exact_div_window.py with -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "../../gr-ldpc_ece535a_amd/csrc/ldpc_exact.hpp"

using namespace ldpc::ex;

namespace {

struct Tally {
  int64_t outside = 0, wrong = 0;
  double lo = INFINITY, hi = -INFINITY;  // extremes of b * yk - 1 (rounded once)
};

// b * yk against the window, exactly: the product is hi + lo with
// hi = RN(b yk), lo = fma(b, yk, -hi) (exact: no operand near the ends of the
// exponent range), and both bounds are doubles
void window(double b, double yk, Tally &t) {
  const double L = 1.0 + 0x1p-41, U = 1.0 + 0x1p-39;
  const double hi = b * yk, lo = fma(b, yk, -hi);
  const bool above = hi > L || (hi == L && lo > 0.0);
  const bool below = hi < U || (hi == U && lo < 0.0);
  if (!(above && below)) ++t.outside;
  const double d = (hi - 1.0) + lo;  // hi - 1 is exact (hi in [1/2, 2])
  if (!(d >= t.lo)) t.lo = d;
  if (!(d <= t.hi)) t.hi = d;
}

template <int k>
void run(const double *a, const double *b, int64_t n, Tally &t) {
  for (int64_t i = 0; i + k <= n; i += k) {
    double x[k], y[k], yk[k], q[k];
    for (int j = 0; j < k; ++j) {
      x[j] = a[i + j];
      y[j] = b[i + j];
    }
    div_recips<k>(y, yk);
    div_n<k>(x, y, q);
    for (int j = 0; j < k; ++j) {
      window(y[j], yk[j], t);
      const double want = x[j] / y[j];
      if (bits(q[j]) != bits(want)) ++t.wrong;
    }
  }
}

}  // namespace

extern "C" {

void set_rcp_perturb(int ulps_) { g_rcp_perturb_ulps = ulps_; }

// div_n<k>, k = 1..3, on consecutive groups of (a, b).  out[0]: products
// outside the window, out[1]: quotients that differ from a / b; ext[0..1]:
// the smallest and largest b * yk - 1 seen.
void check_window(int k, const double *a, const double *b, int64_t n, int64_t *out, double *ext) {
  Tally t;
  if (k == 1)
    run<1>(a, b, n, t);
  else if (k == 2)
    run<2>(a, b, n, t);
  else
    run<3>(a, b, n, t);
  out[0] = t.outside;
  out[1] = t.wrong;
  ext[0] = t.lo;
  ext[1] = t.hi;
}
}
