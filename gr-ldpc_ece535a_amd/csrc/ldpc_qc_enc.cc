// ldpc_qc_enc.cc -- the dual-diagonal quasi-cyclic encoder's form check, step
// program and host executor (host only; see ldpc_qc_enc.hpp).
#include "ldpc_qc_enc.hpp"

#include <stdio.h>

#include <algorithm>

namespace ldpc {

int QcEncProgram::threads() const {
  const int cz = (Z + 63) / 64;
  int steps = 1;
  for (int l = 0; l < levels(); ++l) steps = std::max(steps, level_begin[l + 1] - level_begin[l]);
  // a wave per unit of the widest level, but no more waves than its positions
  // fill (Z below a wave: a unit leaves lanes idle, so the waves take turns)
  const int64_t filled = ((int64_t)steps * Z + 63) / 64;
  return 64 * (int)std::min<int64_t>({(int64_t)steps * cz, filled, (int64_t)kQcEncMaxWaves});
}

bool qc_enc_compile(int mb, int nb, int Z, const int32_t *shifts, QcEncProgram &p,
                    std::string *why) {
  char buf[200];
  auto P = [&](int r, int c) { return shifts[(size_t)r * nb + c]; };
  auto fail = [&](int r, int c, const char *msg) {
    snprintf(buf, sizeof buf, "block row %d, block column %d: %s", r, c, msg);
    if (why) *why = buf;
    return false;
  };
  if (nb <= mb) {
    if (why) *why = "no information block column (nb <= mb)";
    return false;
  }
  // the core is as long as the run of entries just above the diagonal
  int mc = 1;
  while (mc < mb && P(mc - 1, mc) >= 0) ++mc;
  if (mc == 1) mc = 0;
  if (mc == 2)
    return fail(0, 1, "an entry above the diagonal, and no core of at least three block rows");
  int a = -1, b = -1, x = -1;
  if (mc) {
    for (int k = 1; k < mc; ++k)
      for (int r = 0; r < mc; ++r) {
        const bool dual = r == k - 1 || r == k;
        if (dual && P(r, k) != 0)
          return fail(r, k, P(r, k) < 0 ? "the core's dual diagonal lacks this entry"
                                        : "a dual-diagonal entry of the core at a shift other than 0");
        if (!dual && P(r, k) >= 0) return fail(r, k, "a stray entry in the core's dual-diagonal part");
      }
    for (int r = 0; r < mc; ++r)
      for (int c = mc; c < mb; ++c)
        if (P(r, c) >= 0) return fail(r, c, "a core row with an entry in an extension parity column");
    a = P(0, 0);
    if (a < 0) return fail(0, 0, "the core's first parity column lacks its top entry");
    if (P(mc - 1, 0) < 0) return fail(mc - 1, 0, "the core's first parity column lacks its bottom entry");
    if (P(mc - 1, 0) != a) {
      snprintf(buf, sizeof buf,
               "block row %d, block column 0: the bottom shift %d differs from the top shift %d "
               "(they must cancel)",
               mc - 1, P(mc - 1, 0), a);
      if (why) *why = buf;
      return false;
    }
    for (int r = 1; r < mc - 1; ++r)
      if (P(r, 0) >= 0) {
        if (x >= 0) return fail(r, 0, "a fourth entry in the core's first parity column");
        x = r;
        b = P(r, 0);
      }
    if (x < 0) return fail(1, 0, "the core's first parity column has no middle entry");
  }
  for (int r = mc; r < mb; ++r) {
    if (P(r, r) < 0) return fail(r, r, "a missing diagonal entry");
    for (int c = r + 1; c < mb; ++c)
      if (P(r, c) >= 0) return fail(r, c, "an entry right of the diagonal");
  }

  p = QcEncProgram();
  p.mb = mb;
  p.nb = nb;
  p.Z = Z;
  p.core = mc;
  p.scratch = mc;
  // the steps with their levels, then bucketed by level
  struct Draft {
    int level;
    QcEncStep st;
    std::vector<QcEncSrc> src;
  };
  std::vector<Draft> draft;
  std::vector<int> plevel(mb, 0);  // the level that finishes parity block c
  auto info = [&](int r, std::vector<QcEncSrc> &src) {
    for (int c = mb; c < nb; ++c)
      if (P(r, c) >= 0) src.push_back({c, P(r, c)});
  };
  for (int r = 0; r < mb; ++r) {  // level 0: lam_r
    Draft d{0, {r < mc ? nb + r : r, r < mc ? 0 : P(r, r), 0, 0}, {}};
    info(r, d.src);
    draft.push_back(d);
  }
  if (mc) {
    Draft d0{1, {0, b, 0, 0}, {}};
    for (int r = 0; r < mc; ++r) d0.src.push_back({nb + r, 0});
    draft.push_back(d0);
    plevel[0] = 1;
    for (int k = 1; k < mc; ++k) {
      Draft d{2, {k, 0, 0, 0}, {}};
      d.src.push_back({0, a});
      for (int r = 0; r < k; ++r) d.src.push_back({nb + r, 0});
      if (k > x) d.src.push_back({0, b});
      draft.push_back(d);
      plevel[k] = 2;
    }
  }
  int top = mc ? 2 : 0;
  for (int r = mc; r < mb; ++r) {
    Draft d{0, {r, P(r, r), 0, 0}, {}};
    d.src.push_back({r, P(r, r)});  // lam_r, where level 0 left it
    for (int c = 0; c < r; ++c)
      if (P(r, c) >= 0) {
        d.src.push_back({c, P(r, c)});
        d.level = std::max(d.level, plevel[c] + 1);
      }
    plevel[r] = d.level;
    top = std::max(top, d.level);
    if (d.level > 0) draft.push_back(d);  // nothing left of the diagonal: level 0 was all
  }
  for (int l = 0; l <= top; ++l) {
    p.level_begin.push_back((int32_t)p.steps.size());
    for (const Draft &d : draft)
      if (d.level == l) {
        QcEncStep st = d.st;
        st.src_begin = (int32_t)p.srcs.size();
        st.src_count = (int32_t)d.src.size();
        p.srcs.insert(p.srcs.end(), d.src.begin(), d.src.end());
        p.steps.push_back(st);
      }
  }
  p.level_begin.push_back((int32_t)p.steps.size());
  return true;
}

void qc_enc_run(const QcEncProgram &p, const uint8_t *data, int B, uint8_t *cw) {
  const int Z = p.Z;
  const size_t M = (size_t)p.mb * Z, N = (size_t)p.nb * Z, K = N - M;
  std::vector<uint8_t> buf((size_t)(p.nb + p.scratch) * Z);
  for (int f = 0; f < B; ++f) {
    std::fill(buf.begin(), buf.end(), 0);
    for (size_t i = 0; i < K; ++i) buf[M + i] = data[(size_t)f * K + i] & 1;
    for (const QcEncStep &st : p.steps)
      for (int i = 0; i < Z; ++i) {
        uint8_t acc = 0;
        for (int k = 0; k < st.src_count; ++k) {
          const QcEncSrc &s = p.srcs[(size_t)st.src_begin + k];
          acc ^= buf[(size_t)s.block * Z + (i + s.shift) % Z];
        }
        buf[(size_t)st.dst * Z + (i + st.dst_shift) % Z] = acc;
      }
    std::copy(buf.begin(), buf.begin() + N, cw + (size_t)f * N);
  }
}

void qc_enc_pack(const QcEncProgram &p, std::vector<uint32_t> &tab) {
  const uint32_t L = (uint32_t)p.levels(), S0 = 2 + 2 * L;
  const uint32_t src0 = S0 + 3 * (uint32_t)p.steps.size();
  auto word = [&](int block, int shift) {
    return (uint32_t)block * (uint32_t)p.Z | (uint32_t)shift << 20;
  };
  tab.assign(src0, 0);
  tab[0] = L;
  tab[1] = S0;
  for (uint32_t l = 0; l < L; ++l) {
    tab[2 + 2 * l] = (uint32_t)p.level_begin[l];
    tab[3 + 2 * l] = (uint32_t)(p.level_begin[l + 1] - p.level_begin[l]);
  }
  for (size_t s = 0; s < p.steps.size(); ++s) {
    const QcEncStep &st = p.steps[s];
    tab[S0 + 3 * s] = word(st.dst, st.dst_shift);
    tab[S0 + 3 * s + 1] = src0 + (uint32_t)st.src_begin;
    tab[S0 + 3 * s + 2] = (uint32_t)st.src_count;
  }
  for (const QcEncSrc &s : p.srcs) tab.push_back(word(s.block, s.shift));
}

}  // namespace ldpc
