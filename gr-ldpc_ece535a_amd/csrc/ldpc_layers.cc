// ldpc_layers.cc -- layer plan, LDS budget and tables of the layered min-sum
// decoder (host only; see ldpc_layers.hpp).
#include "ldpc_layers.hpp"

#include <stdio.h>

#include <algorithm>

namespace ldpc {
namespace {

constexpr int kRedBytes = 128;

constexpr int64_t al16(int64_t x) { return (x + 15) & ~(int64_t)15; }

}  // namespace

int plan_layers(int M, int N, const int32_t *rp, const int32_t *ci,
                std::vector<int32_t> &layer_of_row) {
  layer_of_row.assign((size_t)M, 0);
  // the layers each column is in so far, and per layer the last row that
  // found it taken
  std::vector<std::vector<int32_t>> of_col((size_t)N);
  std::vector<int32_t> taken_by;
  int L = 0;
  for (int j = 0; j < M; ++j) {
    for (int32_t e = rp[j]; e < rp[j + 1]; ++e)
      for (int32_t l : of_col[ci[e]]) taken_by[l] = j;
    int l = 0;
    while (l < L && taken_by[l] == j) ++l;
    if (l == L) {
      taken_by.push_back(-1);
      ++L;
    }
    layer_of_row[j] = l;
    for (int32_t e = rp[j]; e < rp[j + 1]; ++e) of_col[ci[e]].push_back(l);
  }
  return L;
}

int check_layers(int M, int N, const int32_t *rp, const int32_t *ci, const int32_t *layer_of_row,
                 std::string *why) {
  char buf[160];
  int L = 0;
  for (int j = 0; j < M; ++j) {
    if (layer_of_row[j] < 0 || layer_of_row[j] >= M) {
      snprintf(buf, sizeof buf, "row %d: layer %d is outside [0, %d)", j, layer_of_row[j], M);
      if (why) *why = buf;
      return -1;
    }
    L = std::max(L, layer_of_row[j] + 1);
  }
  // owner[c]: the row that holds column c in layer in_layer[c]; rows are
  // visited layer by layer, ascending within one
  std::vector<int32_t> count((size_t)L + 1, 0), order((size_t)M);
  for (int j = 0; j < M; ++j) count[layer_of_row[j] + 1]++;
  for (int l = 0; l < L; ++l) count[l + 1] += count[l];
  for (int j = 0; j < M; ++j) order[count[layer_of_row[j]]++] = j;
  std::vector<int32_t> in_layer((size_t)N, -1), owner((size_t)N, -1);
  for (int r = 0; r < M; ++r) {
    const int j = order[r], l = layer_of_row[j];
    for (int32_t e = rp[j]; e < rp[j + 1]; ++e) {
      const int c = ci[e];
      if (in_layer[c] == l) {
        snprintf(buf, sizeof buf, "rows %d and %d of layer %d share column %d", owner[c], j, l, c);
        if (why) *why = buf;
        return -1;
      }
      in_layer[c] = l;
      owner[c] = j;
    }
  }
  return L;
}

bool layered_layout(int M, int N, int E, int dc_max, int L, int max_layer_rows, int prec,
                    LayeredLayout &lay) {
  const int64_t real = prec == 1 ? 4 : 8;
  const int64_t r = al16((int64_t)N * real), hard = r + al16((int64_t)E * real);
  const int64_t red = hard + al16(N), frame = red + kRedBytes;
  const int64_t threads = std::min<int64_t>(
      kLayeredMaxThreads, std::max<int64_t>(64, ((int64_t)max_layer_rows + 63) / 64 * 64));
  const bool fits = frame <= kLayeredLdsLimit && M <= kLayeredIndexMax && N <= kLayeredIndexMax &&
                    E <= kLayeredIndexMax && dc_max <= kLayeredDcMax;
  // the tables behind the frame, where there is room for all of them
  const int64_t rows = frame, ci = rows + al16((int64_t)M * 4), order = ci + al16((int64_t)E * 2);
  const int64_t off = order + al16((int64_t)M * 2), staged_total = off + al16(((int64_t)L + 1) * 4);
  const bool staged = fits && staged_total <= kLayeredLdsLimit;
  const int64_t cap = 0x7fffffff;
  lay.r = (int)std::min(r, cap);
  lay.hard = (int)std::min(hard, cap);
  lay.red = (int)std::min(red, cap);
  lay.rows = (int)std::min(rows, cap);
  lay.ci = (int)std::min(ci, cap);
  lay.order = (int)std::min(order, cap);
  lay.off = (int)std::min(off, cap);
  lay.staged = staged ? 1 : 0;
  lay.frame = (int)std::min(frame, cap);
  lay.total = (int)std::min(staged ? staged_total : frame, cap);
  lay.threads = (int)threads;
  return fits;
}

bool layered_q8_layout(int M, int N, int64_t E, int dc_max, int dv_max, int L,
                       int max_layer_rows, int Z, LayeredLayout &lay) {
  const bool tables = Z <= 0;
  const int64_t r = al16((int64_t)N * 2), red = r + al16(E), frame = red + kRedBytes;
  const int64_t threads = std::min<int64_t>(
      kLayeredMaxThreads, std::max<int64_t>(64, ((int64_t)max_layer_rows + 63) / 64 * 64));
  const bool fits = frame <= kLayeredLdsLimit && M <= kLayeredIndexMax && N <= kLayeredIndexMax &&
                    (tables ? E : E / Z) <= kLayeredIndexMax && dc_max <= kLayeredDcMax &&
                    dv_max <= kLayeredQ8DvMax;
  const int64_t rows = frame, ci = rows + al16((int64_t)M * 4), order = ci + al16(E * 2);
  const int64_t off = order + al16((int64_t)M * 2), staged_total = off + al16(((int64_t)L + 1) * 4);
  const bool staged = tables && fits && staged_total <= kLayeredLdsLimit;
  const int64_t cap = 0x7fffffff;
  lay.r = (int)std::min(r, cap);
  lay.hard = lay.red = (int)std::min(red, cap);
  lay.rows = (int)std::min(rows, cap);
  lay.ci = (int)std::min(ci, cap);
  lay.order = (int)std::min(order, cap);
  lay.off = (int)std::min(off, cap);
  lay.staged = staged ? 1 : 0;
  lay.frame = (int)std::min(frame, cap);
  lay.total = (int)std::min(staged ? staged_total : frame, cap);
  lay.threads = (int)threads;
  return fits;
}

void layered_build(int M, const int32_t *rp, const int32_t *ci,
                   const std::vector<int32_t> &layer_of_row, int L, LayeredTables &t) {
  const int E = rp[M];
  t.L = L;
  t.rows.assign((size_t)M, 0);
  t.ci.assign((size_t)E, 0);
  t.order.assign((size_t)M, 0);
  t.off.assign((size_t)L + 1, 0);
  for (int j = 0; j < M; ++j) {
    t.rows[j] = (uint32_t)rp[j] | (uint32_t)(rp[j + 1] - rp[j]) << 16;
    t.off[layer_of_row[j] + 1]++;
  }
  for (int e = 0; e < E; ++e) t.ci[e] = (uint16_t)ci[e];
  for (int l = 0; l < L; ++l) t.off[l + 1] += t.off[l];
  std::vector<uint32_t> fill(t.off.begin(), t.off.end() - 1);
  for (int j = 0; j < M; ++j) t.order[fill[layer_of_row[j]]++] = (uint16_t)j;
}

}  // namespace ldpc
