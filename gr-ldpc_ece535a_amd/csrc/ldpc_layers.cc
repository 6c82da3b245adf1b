// ldpc_layers.cc -- layer plan, LDS budget and tables of the layered min-sum
// decoder (host only; see ldpc_layers.hpp).
#include "ldpc_layers.hpp"

#include <stdio.h>

#include <algorithm>

namespace ldpc {

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

namespace {

// What the two layouts share behind the frame's own regions: the reduction
// words, the tables where there is room for all of them (`stage`: the route
// has tables to stage), the totals and the workgroup's size.
void finish_layout(LdsCarve &c, int M, int64_t E, int L, int max_layer_rows, bool fits, bool stage,
                   LayeredLayout &lay) {
  lay.red = c.take(kWgRedBytes);
  const int64_t frame = c.end;
  lay.rows = c.take((int64_t)M * 4);
  lay.ci = c.take(E * 2);
  lay.order = c.take((int64_t)M * 2);
  lay.off = c.take(((int64_t)L + 1) * 4);
  const bool staged = stage && fits && c.end <= kLayeredLdsLimit;
  lay.staged = staged ? 1 : 0;
  lay.frame = LdsCarve::sat(frame);
  lay.total = LdsCarve::sat(staged ? c.end : frame);
  lay.threads = (int)std::min<int64_t>(
      kLayeredMaxThreads, std::max<int64_t>(64, ((int64_t)max_layer_rows + 63) / 64 * 64));
}

}  // namespace

bool layered_layout(int M, int N, int E, int dc_max, int L, int max_layer_rows, int prec,
                    LayeredLayout &lay) {
  const int64_t real = prec == 1 ? 4 : 8;
  LdsCarve c;
  c.take((int64_t)N * real);  // LQ
  lay.r = c.take((int64_t)E * real);
  lay.hard = c.take(N);
  const bool fits = c.end + kWgRedBytes <= kLayeredLdsLimit && M <= kLayeredIndexMax &&
                    N <= kLayeredIndexMax && E <= kLayeredIndexMax && dc_max <= kLayeredDcMax;
  finish_layout(c, M, E, L, max_layer_rows, fits, true, lay);
  return fits;
}

bool layered_q8_layout(int M, int N, int64_t E, int dc_max, int dv_max, int L,
                       int max_layer_rows, int Z, LayeredLayout &lay) {
  const bool tables = Z <= 0;
  LdsCarve c;
  c.take((int64_t)N * 2);  // LQ
  lay.r = c.take(E);
  lay.hard = LdsCarve::sat(c.end);  // unused: the decisions are read in place
  const bool fits = c.end + kWgRedBytes <= kLayeredLdsLimit && M <= kLayeredIndexMax &&
                    N <= kLayeredIndexMax && (tables ? E : E / Z) <= kLayeredIndexMax &&
                    dc_max <= kLayeredDcMax && dv_max <= kLayeredQ8DvMax;
  finish_layout(c, M, E, L, max_layer_rows, fits, tables, lay);
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
