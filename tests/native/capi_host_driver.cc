// A stand-alone run of the C ABI's pure host code (ldpc_capi_host.cc), for
// building with -fsanitize=address,undefined (make -C gr-ldpc_ece535a_amd
// capi_host_asan).  Arguments: the alist fixtures of tests/golden.  For each:
// parses it into buffers of exactly the reported sizes; on the dense H runs
// ldpc_reorder_h, ldpc_encode of a few fixed data words and ldpc_check_frame
// (every codeword must have syndrome weight 0), the systematic matrix
// (H [A d | d] = 0 for the same words) and the staircase recogniser; then
// parses the text truncated at every 64th byte, with one index replaced by
// N + 1 and by -1, and with a maximum degree whose padded length overflows:
// each must give an error or a consistent matrix.  Exit
// status 0 iff all hold (and the sanitizers stayed silent).
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "ldpc_capi_host.hpp"
#include "ldpc_hip.h"

using namespace ldpc::capi;

namespace {

constexpr int64_t kDenseMax = (int64_t)1 << 24;  // cells of a dense H the driver will hold
constexpr int kWords = 4;

struct Csr {
  int M = 0, N = 0;
  std::vector<int32_t> rp, ci;
};

// The two-call protocol of ldpc_alist_read: sizes first, then buffers of
// exactly those sizes.  >= 0: E, and a matrix that valid_csr accepts; < 0: the
// parser's refusal; -100: an inconsistent result.
int parse(const char *path, Csr &c) {
  const int E = ldpc_alist_read(path, &c.M, &c.N, nullptr, nullptr, 0);
  if (E < 0) return E;
  c.rp.assign((size_t)c.M + 1, -1);
  c.ci.assign((size_t)E, -1);
  int M2 = 0, N2 = 0;
  const int E2 = ldpc_alist_read(path, &M2, &N2, c.rp.data(), c.ci.data(), E);
  if (E2 != E || M2 != c.M || N2 != c.N || c.rp[c.M] != E ||
      !valid_csr(c.M, c.N, c.rp.data(), c.ci.data()))
    return -100;
  return E;
}

bool write_file(const std::string &path, const std::string &text) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return fclose(f) == 0 && ok;
}

// Byte range [b, e) of whitespace-separated token `t` of text (e == b: none).
void token_range(const std::string &text, size_t t, size_t &b, size_t &e) {
  size_t i = 0, n = 0;
  b = e = 0;
  while (i < text.size()) {
    while (i < text.size() && isspace((unsigned char)text[i])) ++i;
    const size_t s = i;
    while (i < text.size() && !isspace((unsigned char)text[i])) ++i;
    if (i > s && n++ == t) {
      b = s;
      e = i;
      return;
    }
  }
}

void fixed_word(int w, int K, uint8_t *d) {
  uint32_t x = 0x2545F491u;
  for (int i = 0; i < K; ++i) {
    x = x * 1664525u + 1013904223u;
    d[i] = w == 0 ? 0 : w == 1 ? 1 : w == 2 ? (uint8_t)(i & 1) : (uint8_t)((x >> 16) & 1);
  }
}

int syndrome_weight(const Csr &c, const uint8_t *bits) {
  int weight = 0;
  for (int j = 0; j < c.M; ++j) {
    int par = 0;
    for (int32_t e = c.rp[j]; e < c.rp[j + 1]; ++e) par ^= bits[c.ci[e]] & 1;
    weight += par;
  }
  return weight;
}

// The dense-H checks of one fixture.
bool check_dense(const char *name, const Csr &c) {
  const int M = c.M, N = c.N, K = N - M;
  std::vector<uint8_t> H((size_t)M * N, 0);
  for (int j = 0; j < M; ++j)
    for (int32_t e = c.rp[j]; e < c.rp[j + 1]; ++e) H[(size_t)j * N + c.ci[e]] = 1;
  std::vector<int32_t> chosen((size_t)M, -1);
  if (ldpc_reorder_h(H.data(), M, N, chosen.data()) != LDPC_OK) {
    fprintf(stderr, "%s: ldpc_reorder_h refused a parsed matrix\n", name);
    return false;
  }
  Csr r;  // the reordered H, for the syndromes
  r.M = M;
  r.N = N;
  dense_to_csr(H.data(), M, N, r.rp, r.ci);
  if (!valid_csr(M, N, r.rp.data(), r.ci.data()) || r.rp[M] != c.rp[M]) {
    fprintf(stderr, "%s: the reordered H is not a column permutation of the parsed one\n", name);
    return false;
  }
  std::vector<uint8_t> data((size_t)kWords * K), cw((size_t)kWords * N, 0xEE);
  for (int w = 0; w < kWords; ++w) fixed_word(w, K, &data[(size_t)w * K]);
  const int enc = ldpc_encode(H.data(), M, N, data.data(), kWords, cw.data());
  if (enc == LDPC_OK) {
    for (int w = 0; w < kWords; ++w) {
      const uint8_t *f = &cw[(size_t)w * N];
      for (int i = 0; i < K; ++i)
        if (f[M + i] != data[(size_t)w * K + i]) {
          fprintf(stderr, "%s word %d: the codeword does not carry its data\n", name, w);
          return false;
        }
      if (ldpc_check_frame(H.data(), M, N, f, M) != 0 || syndrome_weight(r, f) != 0) {
        fprintf(stderr, "%s word %d: ldpc_encode's codeword fails a check\n", name, w);
        return false;
      }
    }
  } else if (N == 2 * M && enc != LDPC_ESINGULAR) {
    // (N != 2M: the reference encoder takes rate-1/2 codes only; singular
    // factors are a property of the code, and reported as such)
    fprintf(stderr, "%s: ldpc_encode returned %d on a reordered H\n", name, enc);
    return false;
  }
  std::vector<uint64_t> A;
  const bool sys = systematic_matrix(H.data(), M, N, A);
  if (sys) {
    const int KW = (K + 63) / 64;
    if (A.size() != (size_t)M * KW) return false;
    std::vector<uint8_t> f((size_t)N);
    for (int w = 0; w < kWords; ++w) {
      const uint8_t *d = &data[(size_t)w * K];
      for (int j = 0; j < M; ++j) {
        int par = 0;
        for (int i = 0; i < K; ++i) par ^= (int)((A[(size_t)j * KW + i / 64] >> (i % 64)) & 1) & d[i];
        f[j] = (uint8_t)par;
      }
      for (int i = 0; i < K; ++i) f[M + i] = d[i];
      if (syndrome_weight(r, f.data()) != 0) {
        fprintf(stderr, "%s word %d: H [A d | d] != 0\n", name, w);
        return false;
      }
    }
  } else if (enc == LDPC_OK) {
    fprintf(stderr, "%s: ldpc_encode solved what systematic_matrix calls dependent\n", name);
    return false;
  }
  const bool stairs = has_staircase(M, r.rp.data(), r.ci.data());
  printf("%s: M %d N %d E %d: encode %d, systematic %d, staircase %d\n", name, M, N, c.rp[M], enc,
         sys ? 1 : 0, stairs ? 1 : 0);
  return true;
}

// Damaged copies of the fixture's text: none may parse to an inconsistent
// matrix (nor, under the sanitizers, read or write out of bounds).
bool check_damaged(const char *name, const std::string &text, const Csr &c, const std::string &tmp) {
  int parsed = 0, refused = 0;
  const auto run = [&](const std::string &t) {
    Csr d;
    if (!write_file(tmp, t)) return false;
    const int rc = parse(tmp.c_str(), d);
    if (rc == -100) return false;
    (rc >= 0 ? parsed : refused) += 1;
    return true;
  };
  for (size_t cut = 0; cut < text.size(); cut += 64)
    if (!run(text.substr(0, cut))) {
      fprintf(stderr, "%s cut at byte %zu: inconsistent parse\n", name, cut);
      return false;
    }
  // the first entry of the column lists and the last token of the row lists
  size_t tokens = 0, b, e;
  for (;; ++tokens) {
    token_range(text, tokens, b, e);
    if (e == b) break;
  }
  const size_t where[2] = {(size_t)4 + c.N + c.M, tokens - 1};
  const std::string bad[2] = {std::to_string(c.N + 1), "-1"};
  for (size_t t : where)
    for (const std::string &v : bad) {
      token_range(text, t, b, e);
      if (e == b) return false;
      if (!run(text.substr(0, b) + v + text.substr(e))) {
        fprintf(stderr, "%s token %zu = %s: inconsistent parse\n", name, t, v.c_str());
        return false;
      }
    }
  // a maximum column degree whose padded length overflows: legal in the
  // unpadded form, refused in the padded one
  token_range(text, 2, b, e);
  if (e == b || !run(text.substr(0, b) + "9223372036854775807" + text.substr(e))) {
    fprintf(stderr, "%s with a huge maximum degree: inconsistent parse\n", name);
    return false;
  }
  printf("%s: %d damaged copies parsed, %d refused\n", name, parsed, refused);
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s tests/golden/*.alist\n", argv[0]);
    return 2;
  }
  char tmp[] = "/tmp/capi_host_XXXXXX";
  const int fd = mkstemp(tmp);
  if (fd < 0) return 2;
  close(fd);
  bool ok = true;
  for (int a = 1; a < argc && ok; ++a) {
    const char *name = argv[a];
    Csr c;
    const int E = parse(name, c);
    if (E < 0) {
      fprintf(stderr, "%s: parse failed (%d): %s\n", name, E, create_error().c_str());
      ok = false;
      break;
    }
    if ((int64_t)c.M * c.N <= kDenseMax) ok = check_dense(name, c);
    std::string text;
    if (FILE *f = fopen(name, "r")) {
      char buf[4096];
      for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
      fclose(f);
    }
    ok = ok && !text.empty() && check_damaged(name, text, c, tmp);
  }
  // a null or unreadable path is refused, not read
  int M, N;
  ok = ok && ldpc_alist_read(nullptr, &M, &N, nullptr, nullptr, 0) == LDPC_EINVAL &&
       ldpc_alist_read("/nonexistent/x.alist", &M, &N, nullptr, nullptr, 0) == LDPC_EINVAL;
  unlink(tmp);
  return ok ? 0 : 1;
}
