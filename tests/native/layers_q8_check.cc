// layers_q8_check.cc -- a stand-alone run of the host-only budget and table
// code behind the fixed-point layered decoder (csrc/ldpc_layers.cc,
// csrc/ldpc_qc.cc), meant to be built with -fsanitize=address,undefined
// (tests/test_layered_q8_host.py does): the layouts of the three large codes,
// the tables of a quasi-cyclic code and of its first-fit plan, every table
// index checked against the sizes the kernels assume.  Exit status 0, or the
// line of the first failed check.
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ldpc_layers.hpp"
#include "ldpc_qc.hpp"

#define CHECK(c)                                       \
  do {                                                 \
    if (!(c)) {                                        \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);  \
      return __LINE__;                                 \
    }                                                  \
  } while (0)

using namespace ldpc;

// mb = 4: the parity part, then `entries` - 7 information entries, block
// column by block column, four to each (bit degrees <= 4).
static std::vector<int32_t> base_of(int nb, int entries) {
  std::vector<int32_t> s((size_t)4 * nb, -1);
  for (int r = 0; r < 4; ++r) {
    s[(size_t)r * nb + r] = 0;
    if (r >= 1) s[(size_t)r * nb + r - 1] = 0;
  }
  int n = 7;
  for (int c = 4; c < nb; ++c)
    for (int r = 0; r < 4; ++r)
      if (n < entries) s[(size_t)r * nb + c] = (37 * n++ + 11) % 1024;
  return s;
}

static int check_code(int nb, int entries, int Z, bool fits_qc, bool fits_tables, int frame) {
  const std::vector<int32_t> s = base_of(nb, entries);
  std::string why;
  CHECK(qc_check(4, nb, Z, s.data(), &why));
  int n, row_max;
  qc_count(4, nb, s.data(), n, row_max);
  CHECK(n == entries);
  const int M = 4 * Z, N = nb * Z;
  const int64_t E = (int64_t)n * Z;
  LayeredLayout lay;
  CHECK(layered_q8_layout(M, N, E, row_max, 4, 4, Z, Z, lay) == fits_qc);
  CHECK(lay.frame == frame && lay.total == frame && !lay.staged && lay.threads == 1024);
  CHECK(lay.r % 16 == 0 && lay.red % 16 == 0 && lay.red - lay.r >= E && lay.r >= 2 * N);
  // the circulant kernel's words: a column below N, a shift below Z, an entry count
  QcTables qt;
  qc_build(4, nb, Z, s.data(), qt);
  CHECK(qt.rows.size() == 4 && qt.ent.size() == (size_t)n + kQcEntPad);
  uint32_t before = 0;
  for (uint32_t rec : qt.rows) {
    CHECK((rec >> 16) == before && (rec & 0xffffu) >= 1 && (rec & 0xffffu) <= (uint32_t)row_max);
    before += rec & 0xffffu;
  }
  CHECK(before == (uint32_t)n);
  for (uint32_t w : qt.ent) CHECK((int)(w & 0xffffu) + Z <= N && (int)(w >> 16) < Z);
  // the table route on the expansion, under first fit
  std::vector<int32_t> rp, ci, plan;
  qc_expand(4, nb, Z, s.data(), rp, ci);
  CHECK((int64_t)ci.size() == E && rp[M] == (int32_t)E);
  const int L = plan_layers(M, N, rp.data(), ci.data(), plan);
  CHECK(check_layers(M, N, rp.data(), ci.data(), plan.data(), &why) == L);
  std::vector<int> rows_of((size_t)L, 0);
  int most = 0;
  for (int32_t l : plan) most = std::max(most, ++rows_of[l]);
  CHECK(layered_q8_layout(M, N, E, row_max, 4, L, most, 0, lay) == fits_tables);
  CHECK(lay.frame == frame && lay.threads <= kLayeredMaxThreads && lay.threads % 64 == 0);
  if (fits_tables) {
    LayeredTables t;
    layered_build(M, rp.data(), ci.data(), plan, L, t);
    CHECK(t.rows.size() == (size_t)M && t.ci.size() == (size_t)E && t.off.size() == (size_t)L + 1);
    CHECK(t.off[L] == (uint32_t)M);
    for (uint16_t j : t.order) CHECK(j < M);
    for (uint32_t rec : t.rows) CHECK((rec & 0xffffu) + (rec >> 16) <= (uint32_t)E);
    if (lay.staged)
      CHECK(lay.total <= kLayeredLdsLimit && lay.rows == lay.frame && lay.ci > lay.rows &&
            lay.order > lay.ci && lay.off > lay.order && lay.total > lay.off);
    else
      CHECK(lay.total == lay.frame);
  }
  return 0;
}

int main() {
  int rc;
  // larger than a float frame; E past 16 bits; the LDS boundary, inside and beyond
  if ((rc = check_code(12, 31, 1024, true, true, 56448))) return rc;
  if ((rc = check_code(24, 67, 1024, true, false, 117888))) return rc;
  if ((rc = check_code(48, 63, 1024, true, true, 162944))) return rc;
  if ((rc = check_code(48, 64, 1024, false, false, 163968))) return rc;
  // degree limits: dc 33, and a bit degree beyond what int16 holds exactly
  LayeredLayout lay;
  CHECK(layered_q8_layout(100, 200, 600, 32, kLayeredQ8DvMax, 3, 40, 0, lay));
  CHECK(!layered_q8_layout(100, 200, 600, 33, 3, 3, 40, 0, lay));
  CHECK(!layered_q8_layout(100, 200, 600, 32, kLayeredQ8DvMax + 1, 3, 40, 0, lay));
  CHECK(127 * (kLayeredQ8DvMax + 1) <= 32767 && 127 * (kLayeredQ8DvMax + 2) > 32767);
  // Z = 1: the base entries are the edges, and the words hold at most 65535 of them
  CHECK(layered_q8_layout(5000, 5001, 65535, 32, 16, 5000, 1, 1, lay));
  CHECK(!layered_q8_layout(5000, 5001, 65536, 32, 16, 5000, 1, 1, lay));
  puts("layers_q8_check ok");
  return 0;
}
