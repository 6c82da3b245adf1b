// ldpc_msn_tables.cc -- host tables of the large-code min-sum pipeline
// (ldpc_graph_msn.hip): the storage order of H's rows and columns and the
// run-length edge descriptors the kernels read (ldpc_graph.hpp: MsnDesc,
// MsnTables).  Host only, no HIP header.
#include <stdlib.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "ldpc_graph.hpp"

namespace ldpc {
namespace {

// H in a storage order, in full: row and column offsets for the degrees, and
// slot-major edge lists (D x n, -1 past the degree) -- rcs[t][p] the storage
// column of row p's t-th edge (ascending original column), crs[t][x] the
// storage row of column x's t-th edge (ascending original row) | the edge's
// place in that row << 24 -- so a wave's t-th edges are one coalesced load.
// Alive only while the descriptors and the contiguity score are built.
struct FullTables {
  std::vector<int32_t> rp, cp, rcs, crs;
};

// Pairs of neighbouring storage rows (columns) of equal degree whose t-th
// edges land on neighbouring storage columns (rows): the contiguity a wave's
// gathers get from the order.
long contiguity(const FullTables &t) {
  long s = 0;
  const int M = (int)t.rp.size() - 1, N = (int)t.cp.size() - 1;
  for (int p = 0; p + 1 < M; ++p) {
    const int d = t.rp[p + 1] - t.rp[p];
    if (t.rp[p + 2] - t.rp[p + 1] != d) continue;
    for (int e = 0; e < d; ++e) s += t.rcs[(size_t)e * M + p + 1] == t.rcs[(size_t)e * M + p] + 1;
  }
  for (int x = 0; x + 1 < N; ++x) {
    const int d = t.cp[x + 1] - t.cp[x];
    if (t.cp[x + 2] - t.cp[x + 1] != d) continue;
    for (int e = 0; e < d; ++e)
      s += (t.crs[(size_t)e * N + x + 1] & 0xffffff) == (t.crs[(size_t)e * N + x] & 0xffffff) + 1;
  }
  return s;
}

// A slot-major table full[t][x] (D x n, -1 past each item's degree) as
// descriptors (MsnDesc: up to 4 runs of consecutive values): S = D per wave
// of the kernels' 256-item blocks, slot t of wave w of block b at
// (4 b + w) S + t; slots past the block's largest degree hold no edge.  Each
// descriptor also carries that degree (pad[0]) and whether its wave's values
// are explicit (pad[1]): a wave with a slot of more than 4 runs keeps every
// slot's 64 values in `x` (at each descriptor's xoff).
void msn_block_tables(const std::vector<int32_t> &full, int D, int n, std::vector<MsnDesc> &desc,
                      std::vector<int32_t> &x) {
  const int nb = (n + kMsnIB - 1) / kMsnIB, nw = kMsnIB / 64, S = D;
  MsnDesc none{};
  for (int r = 0; r < 4; ++r) none.b[r] = kMsnNoEdge;
  none.thr = 64u | 64u << 8 | 64u << 16;
  none.xoff = -1;
  desc.assign((size_t)nb * nw * S, none);
  x.clear();
  for (int b = 0; b < nb; ++b) {
    int deg = 0;
    for (int i = 0; i < kMsnIB; ++i) {
      const int c = b * kMsnIB + i;
      if (c >= n) break;
      for (int t = 0; t < D; ++t)
        if (full[(size_t)t * n + c] != -1) deg = std::max(deg, t + 1);
    }
    for (int w = 0; w < nw; ++w) {
      MsnDesc *mine = &desc[((size_t)b * nw + w) * S];
      std::vector<int32_t> vals((size_t)deg * 64);
      bool explicit_wave = false;
      for (int t = 0; t < deg; ++t) {
        int32_t *v = &vals[(size_t)t * 64];
        for (int l = 0; l < 64; ++l) {
          const int c = b * kMsnIB + w * 64 + l;
          v[l] = c < n ? full[(size_t)t * n + c] : -1;
        }
        int start[64], runs = 0;
        for (int l = 0; l < 64; ++l) {
          const bool cont = l > 0 && ((v[l - 1] < 0 && v[l] < 0) || (v[l - 1] >= 0 && v[l] == v[l - 1] + 1));
          if (!cont) start[runs++] = l;
        }
        MsnDesc &d = mine[t];
        explicit_wave |= runs > 4;
        uint32_t thr = 0;
        for (int r = 0; r < 4; ++r) {
          const int a = r < runs ? start[r] : 64;
          d.b[r] = r < runs ? (v[a] < 0 ? kMsnNoEdge : v[a] - a) : kMsnNoEdge;
          if (r >= 1) thr |= (uint32_t)a << (8 * (r - 1));
        }
        d.thr = thr;
      }
      if (explicit_wave)
        for (int t = 0; t < deg; ++t) mine[t].xoff = (int32_t)(x.size() + (size_t)t * 64);
      if (explicit_wave) x.insert(x.end(), vals.begin(), vals.end());
      for (int t = 0; t < S; ++t) {
        mine[t].pad[0] = deg;
        mine[t].pad[1] = explicit_wave ? 1 : 0;
      }
    }
  }
  // self-check: decode every (block, wave, slot, lane) as the kernels do
  // (desc_words / slot_value / slot_explicit) and compare with the table
  for (int b = 0; b < nb; ++b)
    for (int w = 0; w < nw; ++w)
      for (int t = 0; t < S; ++t) {
        const MsnDesc *mine = &desc[((size_t)b * nw + w) * S];
        const MsnDesc &d = mine[t];
        const int deg = mine[0].pad[0];
        const bool expl = mine[0].pad[1] != 0;
        for (int l = 0; l < 64; ++l) {
          const int c = b * kMsnIB + w * 64 + l;
          const int32_t want = c < n ? full[(size_t)t * n + c] : -1;
          int32_t got;
          if (t >= deg) {
            got = -1;
          } else if (expl) {
            got = x[(size_t)d.xoff + l];
          } else {
            int base = l >= (int)(d.thr & 0xffu) ? d.b[1] : d.b[0];
            base = l >= (int)((d.thr >> 8) & 0xffu) ? d.b[2] : base;
            base = l >= (int)((d.thr >> 16) & 0xffu) ? d.b[3] : base;
            got = base + l;
          }
          if ((want < 0) != (got < 0) || (want >= 0 && want != got))
            throw std::runtime_error("msn_block_tables: descriptor self-check failed");
        }
      }
}

// The tables of H stored with rows at rpos and columns at cpos: the full
// tables as locals, from them the descriptors the kernels read, and the
// order's contiguity, which is returned.
long msn_tables(int M, int N, const std::vector<int32_t> &rp0, const std::vector<int32_t> &ci0,
                const std::vector<int32_t> &rpos, const std::vector<int32_t> &cpos,
                MsnTables &t) {
  FullTables f;
  std::vector<int32_t> rorig(M), corig(N);
  for (int j = 0; j < M; ++j) rorig[rpos[j]] = j;
  for (int c = 0; c < N; ++c) corig[cpos[c]] = c;
  int dc = 0, dv = 0;
  std::vector<int32_t> cdeg((size_t)N, 0);
  for (int j = 0; j < M; ++j) {
    dc = std::max(dc, rp0[j + 1] - rp0[j]);
    for (int32_t o = rp0[j]; o < rp0[j + 1]; ++o) cdeg[cpos[ci0[o]]]++;
  }
  for (int x = 0; x < N; ++x) dv = std::max(dv, cdeg[x]);
  f.rp.assign((size_t)M + 1, 0);
  f.rcs.assign((size_t)dc * M, -1);
  for (int p = 0; p < M; ++p) {
    const int j = rorig[p];
    f.rp[p + 1] = f.rp[p] + (rp0[j + 1] - rp0[j]);
    for (int32_t o = rp0[j]; o < rp0[j + 1]; ++o) f.rcs[(size_t)(o - rp0[j]) * M + p] = cpos[ci0[o]];
  }
  f.cp.assign((size_t)N + 1, 0);
  for (int x = 0; x < N; ++x) f.cp[x + 1] = f.cp[x] + cdeg[x];
  f.crs.assign((size_t)dv * N, -1);
  std::vector<int32_t> fill((size_t)N, 0);
  for (int j = 0; j < M; ++j)  // original rows ascending
    for (int32_t o = rp0[j]; o < rp0[j + 1]; ++o) {
      const int x = cpos[ci0[o]];
      f.crs[(size_t)fill[x]++ * N + x] = rpos[j] | ((o - rp0[j]) << 24);
    }
  t.corig = corig;
  t.cpos = cpos;
  t.rpos = rpos;
  msn_block_tables(f.rcs, dc, M, t.rdesc, t.rx);
  msn_block_tables(f.crs, dv, N, t.cdesc, t.cx);
  t.rs = dc;
  t.cs = dv;
  // outputs from the variable pass need the info columns in place, 8 per byte
  t.out_var = M % 8 == 0;
  for (int c = M; c < N && t.out_var; ++c) t.out_var = cpos[c] == c;
  return contiguity(f);
}

}  // namespace

// Chooses the storage order: the identity, or for M a multiple of 360 the
// DVB-S2 residue-class order (row r -> (r mod q) * 360 + r / q, q = M / 360,
// and the staircase's degree <= 2 columns {r, r+1} moved among their own
// positions in the order of r's class position) -- whichever gives the
// kernels' gathers more contiguity.  LDPC_MSN_ORDER=0 / 1 forces one.
void msn_build(int M, int N, const std::vector<int32_t> &rp0, const std::vector<int32_t> &ci0,
               MsnTables &t) {
  std::vector<int32_t> rid(M), cid(N);
  for (int j = 0; j < M; ++j) rid[j] = j;
  for (int c = 0; c < N; ++c) cid[c] = c;
  const char *env = getenv("LDPC_MSN_ORDER");
  const int force = env ? atoi(env) : -1;
  const long s_id = msn_tables(M, N, rp0, ci0, rid, cid, t);
  t.order = 0;
  t.score[0] = s_id;
  t.score[1] = -1;
  if (M % 360 != 0 || force == 0) return;
  const int q = M / 360;
  std::vector<int32_t> rpos(M), cpos(cid);
  for (int j = 0; j < M; ++j) rpos[j] = (j % q) * 360 + j / q;
  // staircase columns: degree 1 or 2 with rows r (and r + 1)
  std::vector<int32_t> cdeg(N, 0), cfirst(N, -1), clast(N, -1);
  for (int j = 0; j < M; ++j)
    for (int32_t o = rp0[j]; o < rp0[j + 1]; ++o) {
      const int c = ci0[o];
      if (cfirst[c] < 0) cfirst[c] = j;
      clast[c] = j;
      cdeg[c]++;
    }
  std::vector<int32_t> stair, slots;
  for (int c = 0; c < N; ++c)
    if ((cdeg[c] == 1) || (cdeg[c] == 2 && clast[c] == cfirst[c] + 1)) {
      stair.push_back(c);
      slots.push_back(c);
    }
  std::stable_sort(stair.begin(), stair.end(),
                   [&](int a, int b) { return rpos[cfirst[a]] < rpos[cfirst[b]]; });
  for (size_t i = 0; i < stair.size(); ++i) cpos[stair[i]] = slots[i];
  MsnTables qc;
  const long s_qc = msn_tables(M, N, rp0, ci0, rpos, cpos, qc);
  qc.order = 1;
  qc.score[0] = s_id;
  qc.score[1] = s_qc;
  t.score[1] = s_qc;
  if (force == 1 || s_qc > s_id) t = std::move(qc);
}

}  // namespace ldpc
