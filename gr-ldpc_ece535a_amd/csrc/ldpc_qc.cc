// ldpc_qc.cc -- quasi-cyclic codes: check, expansion and the circulant
// kernel's base tables (host only; see ldpc_qc.hpp).
#include "ldpc_qc.hpp"

#include <stdio.h>

#include <algorithm>

namespace ldpc {

bool qc_check(int mb, int nb, int Z, const int32_t *shifts, std::string *why) {
  char buf[160];
  auto fail = [&](const char *msg) {
    if (why) *why = msg;
    return false;
  };
  if (mb < 1 || nb < 1) return fail("a base matrix has at least one row and one column");
  if (Z < 1 || Z > kQcZMax) {
    snprintf(buf, sizeof buf, "the lifting size Z = %d is outside [1, %d]", Z, kQcZMax);
    return fail(buf);
  }
  if (!shifts) return fail("null base matrix");
  int64_t entries = 0;
  for (int64_t p = 0; p < (int64_t)mb * nb; ++p) {
    if (shifts[p] < -1 || shifts[p] >= Z) {
      snprintf(buf, sizeof buf, "base entry (%d, %d): shift %d is outside [-1, %d)",
               (int)(p / nb), (int)(p % nb), shifts[p], Z);
      return fail(buf);
    }
    entries += shifts[p] >= 0;
  }
  const int64_t lim = 0x7fffffff;
  if ((int64_t)mb * Z >= lim || (int64_t)nb * Z >= lim || entries * Z >= lim)
    return fail("the expanded matrix is too large");
  return true;
}

void qc_count(int mb, int nb, const int32_t *shifts, int &entries, int &row_max) {
  entries = row_max = 0;
  for (int r = 0; r < mb; ++r) {
    int d = 0;
    for (int c = 0; c < nb; ++c) d += shifts[(size_t)r * nb + c] >= 0;
    entries += d;
    row_max = std::max(row_max, d);
  }
}

void qc_expand(int mb, int nb, int Z, const int32_t *shifts, std::vector<int32_t> &rp,
               std::vector<int32_t> &ci) {
  int entries, row_max;
  qc_count(mb, nb, shifts, entries, row_max);
  rp.assign((size_t)mb * Z + 1, 0);
  ci.clear();
  ci.reserve((size_t)entries * Z);
  for (int r = 0; r < mb; ++r)
    for (int i = 0; i < Z; ++i) {
      for (int c = 0; c < nb; ++c) {
        const int32_t s = shifts[(size_t)r * nb + c];
        if (s >= 0) ci.push_back(c * Z + (i + s) % Z);
      }
      rp[(size_t)r * Z + i + 1] = (int32_t)ci.size();
    }
}

void qc_build(int mb, int nb, int Z, const int32_t *shifts, QcTables &t) {
  t.rows.clear();
  t.ent.clear();
  for (int r = 0; r < mb; ++r) {
    const uint32_t eb = (uint32_t)t.ent.size();
    for (int c = 0; c < nb; ++c) {
      const int32_t s = shifts[(size_t)r * nb + c];
      if (s >= 0) t.ent.push_back((uint32_t)(c * Z) | (uint32_t)s << 16);
    }
    if (t.ent.size() > eb) t.rows.push_back(((uint32_t)t.ent.size() - eb) | eb << 16);
  }
  t.ent.insert(t.ent.end(), kQcEntPad, 0u);
}

}  // namespace ldpc
