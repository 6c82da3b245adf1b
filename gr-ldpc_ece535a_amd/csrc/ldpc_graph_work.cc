// ldpc_graph_work.cc -- the large-code workspaces (host): each one's regions
// written once, as a walk through an Arena (ldpc_arena.hpp) that fills the
// struct the kernels take.  Over a null base the walk measures the workspace,
// over the buffer it carves it, so the two cannot disagree.
#include <stdlib.h>

#include "ldpc_arena.hpp"
#include "ldpc_graph.hpp"

namespace ldpc {
namespace {

size_t graph_work_walk(GraphWork &w, void *base, const GraphView &g, int Bp, int prec, int method,
                       bool want_post) {
  const size_t real = prec == 1 ? 4 : 8;
  const bool soft = method == 0 || method == 1;
  const size_t chunks = (size_t)Bp / 64, B = (size_t)Bp, N = (size_t)g.N;
  Arena a(base);
  w = GraphWork{};
  w.Bp = Bp;
  w.chunks = (int)chunks;
  w.check_waves = graph_check_waves(g.M);
  if (soft) {
    w.Q = a.take<char>((size_t)g.E * B * real);
    w.R = a.take<char>((size_t)g.E * B * real);
    w.L = a.take<float>(N * B);
  }
  w.hard = a.take<uint64_t>(N * chunks);
  if (!soft) {
    w.y = a.take<uint64_t>(N * chunks);
    w.rowpar = a.take<uint64_t>((size_t)g.M * chunks);
  }
  w.synd_part = a.take<uint64_t>((size_t)w.check_waves * chunks);
  w.done_w = a.take<uint64_t>(chunks);
  w.chunk_done = a.take<uint8_t>(chunks);
  w.used = a.take<int32_t>(B);
  w.synd = a.take<int32_t>(B);
  if (want_post) w.post = a.take<float>(N * B);
  // compaction: state, slot maps, plan, spare hard / L / post
  w.st = a.take<GraphState>(1);
  w.perm = a.take<int32_t>(B);
  w.perm2 = a.take<int32_t>(B);
  w.src = a.take<int32_t>(B);
  w.hard2 = a.take<uint64_t>(N * chunks);
  if (soft) {
    w.L2 = a.take<float>(N * B);
    if (want_post) w.post2 = a.take<float>(N * B);
  }
  return a.bytes();
}

size_t msn_work_walk(MsnWork &w, void *base, const MsnView &g, int chunks, int prec) {
  const size_t real = prec == 1 ? 4 : 8, F = kMsnFrames, C = (size_t)chunks;
  const size_t M = (size_t)g.M, N = (size_t)g.N;
  Arena a(base);
  w = MsnWork{};
  w.chunks = chunks;
  w.S = chunks * kMsnFrames;
  w.real_bytes = (int)real;
  w.nb_check = (g.M + kMsnIB - 1) / kMsnIB;
  w.nb_var = (g.N + kMsnIB - 1) / kMsnIB;
  w.out_var = g.out_var;
  w.L = a.take<float>(C * N * F);
  w.LQ = a.take<char>(C * N * F * real);
  w.m1 = a.take<char>(C * M * F * real);
  w.m2 = a.take<char>(C * M * F * real);
  w.meta = a.take<uint8_t>(C * M * F);
  w.alpha = a.take<uint8_t>(C * msn_alpha_rows(g.dc_max) * M);
  w.capsyn = a.take<int32_t>(C * F);
  w.it = a.take<int32_t>(C * F);
  w.frame = a.take<int32_t>(C * F);
  w.out_frame = a.take<int32_t>(C * F);
  w.used = a.take<int32_t>(C * F);
  w.live = a.take<uint32_t>(2 * C);
  w.run = a.take<uint32_t>(2 * C);
  w.stop = a.take<uint32_t>(2 * C);
  w.fill = a.take<uint32_t>(2 * C);
  // The decision in the check pass's last block per chunk (12-bit arrival
  // counts: M <= kMsnMaxRows).  One word per chunk made the 127 blocks of a
  // chunk contend (check pass 53.5 us against 40.8 + 4.9 for the check and
  // decision launches, profiles/round3/msn/fused_decide.txt); two levels (8
  // group words, then the chunk's) measured 2 219-2 229 against 2 207-2 212
  // Mbit/s for a separate decision launch (profiles/round3/msn/ab_fuse2.txt),
  // which was then removed
  w.arrive = a.take<uint64_t>(C * 9);
  w.ctrl = a.take<int32_t>(16);
  return a.bytes();
}

}  // namespace

size_t graph_work_bytes(const GraphView &g, int Bp, int prec, int method, bool want_post) {
  GraphWork w;
  return graph_work_walk(w, nullptr, g, Bp, prec, method, want_post);
}

void graph_work_carve(GraphWork &w, void *base, const GraphView &g, int Bp, int prec, int method,
                      bool want_post) {
  graph_work_walk(w, base, g, Bp, prec, method, want_post);
}

int msn_default_chunks() {
  const char *e = getenv("LDPC_MSN_CHUNKS");  // A/B knob
  const int v = e ? atoi(e) : 0;
  // 80 chunks of 2 frames = 160 frames in flight, 10 chunks per XCD:
  // 2 518-2 522 Mbit/s against 2 486 for 64, 2 469 for 96 and 2 104 for 112
  // (profiles/round4/msn_chunks/; round 3 at 4 frames per chunk: 40 chunks,
  // profiles/round3/msn/chunks_fused.txt)
  return v >= 1 ? v : 80;
}

size_t msn_work_bytes(const MsnView &g, int chunks, int prec) {
  MsnWork w;
  return msn_work_walk(w, nullptr, g, chunks, prec);
}

void msn_work_carve(MsnWork &w, void *base, const MsnView &g, int chunks, int prec) {
  msn_work_walk(w, base, g, chunks, prec);
}

}  // namespace ldpc
