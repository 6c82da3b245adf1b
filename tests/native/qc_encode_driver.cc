// A stand-alone run of the quasi-cyclic encoder's host code (ldpc_qc_enc.cc,
// ldpc_qc.cc), for building with -fsanitize=address,undefined (make -C
// gr-ldpc_ece535a_amd qc_encode_asan).  Reads the cases tests/qc_encode_cases.py
// writes -- "mb nb Z B", the shifts, B rows of K bits -- and for each: checks
// the description, compiles and packs the step program, checks every table
// word against the LDS the program declares, encodes, and verifies the data
// part and the syndrome on the expanded matrix.  Exit status 0 iff all pass.
#include <stdio.h>

#include <string>
#include <vector>

#include "ldpc_qc.hpp"
#include "ldpc_qc_enc.hpp"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int mb, nb, Z, B, cases = 0;
  while (fscanf(f, "%d %d %d %d", &mb, &nb, &Z, &B) == 4) {
    std::vector<int32_t> shifts((size_t)mb * nb);
    for (auto &s : shifts)
      if (fscanf(f, "%d", &s) != 1) return 2;
    const size_t M = (size_t)mb * Z, N = (size_t)nb * Z, K = N - M;
    std::vector<uint8_t> data((size_t)B * K), cw((size_t)B * N);
    std::string row(K + 1, '\0');
    for (int b = 0; b < B; ++b) {
      if (fscanf(f, "%s", &row[0]) != 1) return 2;
      for (size_t i = 0; i < K; ++i) data[(size_t)b * K + i] = (uint8_t)(row[i] - '0');
    }
    std::string why;
    ldpc::QcEncProgram p;
    if (!ldpc::qc_check(mb, nb, Z, shifts.data(), &why) ||
        !ldpc::qc_enc_compile(mb, nb, Z, shifts.data(), p, &why)) {
      fprintf(stderr, "case %d: %s\n", cases, why.c_str());
      return 1;
    }
    std::vector<uint32_t> tab;
    ldpc::qc_enc_pack(p, tab);
    const uint32_t S0 = tab[1];
    for (uint32_t l = 0; l < tab[0]; ++l)
      for (uint32_t s = tab[2 + 2 * l]; s < tab[2 + 2 * l] + tab[3 + 2 * l]; ++s) {
        const uint32_t *st = &tab.at(S0 + 3 * s);
        for (uint32_t k = 0; k <= st[2]; ++k) {   // the sources, then the destination
          const uint32_t w = k < st[2] ? tab.at(st[1] + k) : st[0];
          if ((w >> 20) >= (uint32_t)Z || (int64_t)(w & 0xFFFFF) + Z > p.lds_bytes()) {
            fprintf(stderr, "case %d: table word outside the frame\n", cases);
            return 1;
          }
        }
      }
    ldpc::qc_enc_run(p, data.data(), B, cw.data());
    std::vector<int32_t> rp, ci;
    ldpc::qc_expand(mb, nb, Z, shifts.data(), rp, ci);
    for (int b = 0; b < B; ++b) {
      const uint8_t *c = &cw[(size_t)b * N];
      for (size_t i = 0; i < K; ++i)
        if (c[M + i] != data[(size_t)b * K + i]) return 1;
      for (size_t j = 0; j < M; ++j) {
        int par = 0;
        for (int32_t e = rp[j]; e < rp[j + 1]; ++e) par ^= c[ci[e]];
        if (par) {
          fprintf(stderr, "case %d frame %d: check %zu fails\n", cases, b, j);
          return 1;
        }
      }
    }
    printf("case %d: mb %d nb %d Z %d core %d levels %d threads %d lds %lld ok\n", cases, mb, nb, Z,
           p.core, p.levels(), p.threads(), (long long)p.lds_bytes());
    ++cases;
  }
  return cases > 0 ? 0 : 2;
}
