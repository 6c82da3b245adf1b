// A stand-alone run of the large-code path's host code (the workspace layouts
// of ldpc_graph_work.cc, the pipeline tables of ldpc_msn_tables.cc), for
// building with -fsanitize=address,undefined (make -C gr-ldpc_ece535a_amd
// large_code_asan).
//
// Workspaces.  Each case is measured over a null base and, where it is small,
// carved into a host buffer of exactly that many bytes: every non-null region
// must be 256-aligned, the regions -- each with the bytes the kernels index,
// restated here -- must ascend without overlap in the order the struct is
// laid out, the last must end within the buffer, and the total must equal the
// literal recorded here.  The literals (and the two offset
// lists) were taken from the parent of the commit that introduced the arena
// walk, by running its graph_work_bytes / graph_work_carve / msn_work_bytes /
// msn_work_carve on the same cases: the sizes and offsets must never move.
//
// Tables.  Reads the CSRs tests/large_code_cases.py writes -- "M N E", the
// M + 1 row offsets, the E columns -- and runs msn_build on each with
// LDPC_MSN_ORDER unset, 0 and 1 (the descriptors' self-check included: an
// exception fails the run), printing the order, the scores, rpos and cpos for
// tests/test_large_code_host.py to compare with the library's.
// Exit status 0 iff all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <exception>
#include <vector>

#include "ldpc_graph.hpp"

namespace {

int failures = 0;

void fail(const char *what, int a, int b, int c, int d, int e) {
  printf("FAIL %s (%d %d %d %d %d)\n", what, a, b, c, d, e);
  ++failures;
}

// a region as the kernels use it: where it starts and the bytes they index
struct Region {
  const char *name;
  const void *p;
  size_t bytes;
};
typedef std::vector<Region> Regions;

// Every non-null region 256-aligned, the regions ascending in the struct's
// order from the base, none reaching into the next, and the last one's end,
// rounded up to 256, exactly the end of the `total` bytes at base.
bool regions_ok(const Regions &r, const char *base, size_t total) {
  const char *end = base;  // of the regions so far
  for (const Region &x : r) {
    const char *p = (const char *)x.p;
    if (!p) continue;
    if ((size_t)(p - base) % 256 != 0 || p < end || (end == base && p != base)) {
      printf("  %s misplaced\n", x.name);
      return false;
    }
    end = p + x.bytes;
    if ((size_t)(end - base) > total) {
      printf("  %s ends past the buffer\n", x.name);
      return false;
    }
  }
  return ((size_t)(end - base) + 255) / 256 * 256 == total;
}

Regions graph_regions(const ldpc::GraphWork &w, const ldpc::GraphView &g, int prec) {
  const size_t real = prec == 1 ? 4 : 8, B = (size_t)w.Bp, C = (size_t)w.chunks, N = (size_t)g.N;
  return {{"Q", w.Q, (size_t)g.E * B * real},
          {"R", w.R, (size_t)g.E * B * real},
          {"L", w.L, N * B * 4},
          {"hard", w.hard, N * C * 8},
          {"y", w.y, N * C * 8},
          {"rowpar", w.rowpar, (size_t)g.M * C * 8},
          {"synd_part", w.synd_part, (size_t)w.check_waves * C * 8},
          {"done_w", w.done_w, C * 8},
          {"chunk_done", w.chunk_done, C},
          {"used", w.used, B * 4},
          {"synd", w.synd, B * 4},
          {"post", w.post, N * B * 4},
          {"st", w.st, sizeof(ldpc::GraphState)},
          {"perm", w.perm, B * 4},
          {"perm2", w.perm2, B * 4},
          {"src", w.src, B * 4},
          {"hard2", w.hard2, N * C * 8},
          {"L2", w.L2, N * B * 4},
          {"post2", w.post2, N * B * 4}};
}

Regions msn_regions(const ldpc::MsnWork &w, const ldpc::MsnView &g) {
  const size_t real = (size_t)w.real_bytes, F = ldpc::kMsnFrames, C = (size_t)w.chunks,
               M = (size_t)g.M, N = (size_t)g.N;
  return {{"L", w.L, C * N * F * 4},
          {"LQ", w.LQ, C * N * F * real},
          {"m1", w.m1, C * M * F * real},
          {"m2", w.m2, C * M * F * real},
          {"meta", w.meta, C * M * F},
          {"alpha", w.alpha, C * (size_t)((g.dc_max + 1) / 2) * M},  // a nibble per edge and chunk
          {"capsyn", w.capsyn, C * F * 4},
          {"it", w.it, C * F * 4},
          {"frame", w.frame, C * F * 4},
          {"out_frame", w.out_frame, C * F * 4},
          {"used", w.used, C * F * 4},
          {"live", w.live, 2 * C * 4},
          {"run", w.run, 2 * C * 4},
          {"stop", w.stop, 2 * C * 4},
          {"fill", w.fill, 2 * C * 4},
          {"arrive", w.arrive, C * 9 * 8},
          {"ctrl", w.ctrl, 8}};
}

bool offsets_are(const Regions &r, const char *base, const std::vector<long> &want) {
  if (r.size() != want.size()) return false;
  for (size_t i = 0; i < r.size(); ++i) {
    const long got = r[i].p ? (long)((const char *)r[i].p - base) : -1;
    if (got != want[i]) {
      printf("  %s at %ld, recorded %ld\n", r[i].name, got, want[i]);
      return false;
    }
  }
  return true;
}

constexpr size_t kCarveLimit = (size_t)4 << 20;  // carve what fits in 4 MiB

// the reference decoder's 32 x 64 H, reordered: 168 edges, row degree 6
constexpr int kRefM = 32, kRefN = 64, kRefE = 168, kRefDc = 6;
// the DVB-S2-size shape of config 4
constexpr int kDvbM = 32400, kDvbN = 64800, kDvbE = 226799;

struct GraphCase {
  int big, Bp, method, prec, want_post;
  unsigned long long bytes;
};
const GraphCase kGraphCases[] = {
    {0, 64, 1, 0, 0, 208128ull},
    {0, 64, 1, 0, 1, 240896ull},
    {0, 64, 1, 1, 0, 122112ull},
    {0, 64, 1, 1, 1, 154880ull},
    {0, 64, 2, 0, 0, 4096ull},
    {0, 64, 2, 0, 1, 20480ull},
    {0, 64, 2, 1, 0, 4096ull},
    {0, 64, 2, 1, 1, 20480ull},
    {0, 64, 3, 0, 0, 4096ull},
    {0, 64, 3, 0, 1, 20480ull},
    {0, 64, 3, 1, 0, 4096ull},
    {0, 64, 3, 1, 1, 20480ull},
    {0, 192, 1, 0, 0, 622336ull},
    {0, 192, 1, 0, 1, 720640ull},
    {0, 192, 1, 1, 0, 364288ull},
    {0, 192, 1, 1, 1, 462592ull},
    {0, 192, 2, 0, 0, 10240ull},
    {0, 192, 2, 0, 1, 59392ull},
    {0, 192, 2, 1, 0, 10240ull},
    {0, 192, 2, 1, 1, 59392ull},
    {0, 192, 3, 0, 0, 10240ull},
    {0, 192, 3, 0, 1, 59392ull},
    {0, 192, 3, 1, 0, 10240ull},
    {0, 192, 3, 1, 1, 59392ull},
    // sizes only: E * Bp * 8 is past 2^32 here, so a narrowed product shows
    {1, 1024, 1, 0, 0, 4264363264ull},
    {1, 4096, 1, 0, 0, 17057451008ull},
};

struct MsnCase {
  int M, N, dc_max, chunks, prec;
  unsigned long long bytes;
};
const MsnCase kMsnCases[] = {
    {kRefM, kRefN, kRefDc, 1, 0, 5888ull},
    {kRefM, kRefN, kRefDc, 1, 1, 4864ull},
    {kRefM, kRefN, kRefDc, 5, 0, 16896ull},
    {kRefM, kRefN, kRefDc, 5, 1, 11776ull},
    {kRefM, kRefN, kRefDc, 8, 0, 25088ull},
    {kRefM, kRefN, kRefDc, 8, 1, 16896ull},
    {kRefM, kRefN, kRefDc, 80, 0, 230656ull},
    {kRefM, kRefN, kRefDc, 80, 1, 148736ull},
    // dc_max 7 and 8 round to the same 4 alpha bytes per row
    {kDvbM, kDvbN, 7, 1, 0, 2789632ull},
    {kDvbM, kDvbN, 7, 1, 1, 1753088ull},
    {kDvbM, kDvbN, 7, 5, 0, 13935360ull},
    {kDvbM, kDvbN, 7, 5, 1, 8751616ull},
    {kDvbM, kDvbN, 7, 8, 0, 22294528ull},
    {kDvbM, kDvbN, 7, 8, 1, 14000128ull},
    {kDvbM, kDvbN, 7, 80, 0, 222925056ull},
    {kDvbM, kDvbN, 7, 80, 1, 139981056ull},
    {kDvbM, kDvbN, 8, 1, 0, 2789632ull},
    {kDvbM, kDvbN, 8, 1, 1, 1753088ull},
    {kDvbM, kDvbN, 8, 5, 0, 13935360ull},
    {kDvbM, kDvbN, 8, 5, 1, 8751616ull},
    {kDvbM, kDvbN, 8, 8, 0, 22294528ull},
    {kDvbM, kDvbN, 8, 8, 1, 14000128ull},
    {kDvbM, kDvbN, 8, 80, 0, 222925056ull},
    {kDvbM, kDvbN, 8, 80, 1, 139981056ull},
};

int workspaces() {
  int n = 0, carved = 0;
  for (const GraphCase &c : kGraphCases) {
    ldpc::GraphView g{};
    g.M = c.big ? kDvbM : kRefM;
    g.N = c.big ? kDvbN : kRefN;
    g.E = c.big ? kDvbE : kRefE;
    const size_t bytes = ldpc::graph_work_bytes(g, c.Bp, c.prec, c.method, c.want_post != 0);
    if (bytes != c.bytes) fail("graph total", c.big, c.Bp, c.method, c.prec, c.want_post);
    ++n;
    if (bytes > kCarveLimit) continue;
    std::vector<char> buf(bytes + 256);  // the exact size, from a 256-aligned start
    char *base = buf.data() + (256 - (uintptr_t)buf.data() % 256) % 256;
    ldpc::GraphWork w;
    ldpc::graph_work_carve(w, base, g, c.Bp, c.prec, c.method, c.want_post != 0);
    if (!regions_ok(graph_regions(w, g, c.prec), base, bytes))
      fail("graph regions", c.big, c.Bp, c.method, c.prec, c.want_post);
    // what a method does not use stays null
    const bool soft = c.method == 1;
    if (soft != (w.Q && w.R && w.L && w.L2) || soft == (w.y && w.rowpar) || !w.hard || !w.st ||
        (c.want_post != 0) != (w.post != nullptr) || (soft && c.want_post) != (w.post2 != nullptr))
      fail("graph conditions", c.big, c.Bp, c.method, c.prec, c.want_post);
    if (w.Bp != c.Bp || w.chunks != c.Bp / 64 || w.check_waves != ldpc::graph_check_waves(g.M))
      fail("graph scalars", c.big, c.Bp, c.method, c.prec, c.want_post);
    if (!c.big && c.Bp == 192 && c.method == 1 && c.prec == 0 && c.want_post &&
        !offsets_are(graph_regions(w, g, c.prec), base,
                     {0, 258048, 516096, 565248, -1, -1, 566784, 567040, 567296, 567552, 568320,
                      569088, 618240, 618496, 619264, 620032, 620800, 622336, 671488}))
      fail("graph offsets", c.big, c.Bp, c.method, c.prec, c.want_post);
    ++carved;
  }
  for (const MsnCase &c : kMsnCases) {
    ldpc::MsnView v{};
    v.M = c.M;
    v.N = c.N;
    v.dc_max = c.dc_max;
    v.out_var = 1;
    const size_t bytes = ldpc::msn_work_bytes(v, c.chunks, c.prec);
    if (bytes != c.bytes) fail("msn total", c.M, c.N, c.dc_max, c.chunks, c.prec);
    ++n;
    if (bytes > kCarveLimit) continue;
    std::vector<char> buf(bytes + 256);
    char *base = buf.data() + (256 - (uintptr_t)buf.data() % 256) % 256;
    ldpc::MsnWork w;
    ldpc::msn_work_carve(w, base, v, c.chunks, c.prec);
    if (!regions_ok(msn_regions(w, v), base, bytes))
      fail("msn regions", c.M, c.N, c.dc_max, c.chunks, c.prec);
    if (w.chunks != c.chunks || w.S != c.chunks * ldpc::kMsnFrames ||
        w.real_bytes != (c.prec == 1 ? 4 : 8) || w.nb_check != (c.M + 255) / 256 ||
        w.nb_var != (c.N + 255) / 256 || w.out_var != 1)
      fail("msn scalars", c.M, c.N, c.dc_max, c.chunks, c.prec);
    if (c.M == kRefM && c.chunks == 5 && c.prec == 0 &&
        !offsets_are(msn_regions(w, v), base,
                     {0, 2560, 7680, 10240, 12800, 13312, 13824, 14080, 14336, 14592, 14848, 15104,
                      15360, 15616, 15872, 16128, 16640}))
      fail("msn offsets", c.M, c.N, c.dc_max, c.chunks, c.prec);
    ++carved;
  }
  printf("workspaces %d carved %d\n", n, carved);
  return n;
}

bool read_ints(std::vector<int32_t> &v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i)
    if (scanf("%d", &v[i]) != 1) return false;
  return true;
}

void print_ints(const char *name, const std::vector<int32_t> &v) {
  printf("%s", name);
  for (int32_t x : v) printf(" %d", x);
  printf("\n");
}

int tables() {
  int cases = 0, M, N, E;
  while (scanf("%d %d %d", &M, &N, &E) == 3) {
    std::vector<int32_t> rp, ci;
    if (M < 1 || N <= M || E < 1 || !read_ints(rp, (size_t)M + 1) || !read_ints(ci, (size_t)E) ||
        rp[M] != E) {
      fail("bad case text", cases, M, N, E, 0);
      return cases;
    }
    const char *const force[3] = {nullptr, "0", "1"};
    for (const char *f : force) {
      if (f)
        setenv("LDPC_MSN_ORDER", f, 1);
      else
        unsetenv("LDPC_MSN_ORDER");
      ldpc::MsnTables t;
      try {
        ldpc::msn_build(M, N, rp, ci, t);
      } catch (const std::exception &ex) {
        printf("FAIL case %d order %s: %s\n", cases, f ? f : "unset", ex.what());
        ++failures;
        continue;
      }
      // what the kernels index by: one descriptor per slot of every wave
      const size_t rw = (size_t)((M + ldpc::kMsnIB - 1) / ldpc::kMsnIB) * 4,
                   cw = (size_t)((N + ldpc::kMsnIB - 1) / ldpc::kMsnIB) * 4;
      if (t.rdesc.size() != rw * t.rs || t.cdesc.size() != cw * t.cs || t.rx.size() % 64 != 0 ||
          t.cx.size() % 64 != 0 || t.corig.size() != (size_t)N || t.cpos.size() != (size_t)N ||
          t.rpos.size() != (size_t)M)
        fail("table sizes", cases, M, N, t.rs, t.cs);
      printf("case %d force %s order %d score %ld %ld out_var %d rs %d cs %d explicit %zu %zu\n",
             cases, f ? f : "unset", t.order, t.score[0], t.score[1], t.out_var ? 1 : 0, t.rs, t.cs,
             t.rx.size() / 64, t.cx.size() / 64);
      print_ints("rpos", t.rpos);
      print_ints("cpos", t.cpos);
    }
    ++cases;
  }
  unsetenv("LDPC_MSN_ORDER");
  printf("tables %d\n", cases);
  return cases;
}

}  // namespace

int main() {
  workspaces();
  tables();
  printf(failures ? "FAILED %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
