// ldpc_qc.hpp -- quasi-cyclic codes for the layered decoder: the description
// (a base matrix of circulant shifts and a lifting size), its expansion to
// CSR, and the base tables of the circulant route (ldpc_layered.hip).
// Host only, no device needed.
//
// A QC code is (mb, nb, Z, shifts): shifts is mb x nb, row-major; -1 is the
// zero block, s in [0, Z) the Z x Z identity rotated by s, so that row
// r * Z + i of H has a one in column c * Z + (i + s) mod Z for every base
// entry (r, c) with s >= 0.  One circulant per cell.  The rows of a block row
// share no column, so the block rows are a layer plan (ldpc_layers.hpp):
// layer_of_row[j] = j / Z.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace ldpc {

constexpr int kQcZMax = 1024;  // a block row is one layer: a thread per row

// Checks a description: mb, nb, Z >= 1, Z <= kQcZMax, every shift in [-1, Z),
// and M, N, E within an int.  False with the reason in *why.
bool qc_check(int mb, int nb, int Z, const int32_t *shifts, std::string *why);

// Base entries >= 0 in all, and the largest number in one base row.
void qc_count(int mb, int nb, const int32_t *shifts, int &entries, int &row_max);

// The expanded H as CSR: rp gets mb * Z + 1 entries, ci Z * entries, the
// columns of a row ascending (ascending block column).
void qc_expand(int mb, int nb, int Z, const int32_t *shifts, std::vector<int32_t> &rp,
               std::vector<int32_t> &ci);

// What the circulant kernel reads, one word per base row and per base entry:
//   rows[r] = d_r | eb_r << 16    the base entries of block row r and those
//                                  before it (eb_r = d_0 + ... + d_{r-1}); block
//                                  rows without any are left out (nothing to
//                                  update, always satisfied), so every d_r >= 1
//   ent[eb_r + k] = c_k * Z | s_k << 16   the row's entries in ascending c_k
// (a code that fits the layered kernels has N <= 65535 and at most 65535 base
// entries -- the float kernels through E <= 65535, the fixed-point one through
// layered_q8_layout's E / Z <= 65535 -- so c * Z and the number of entries fit
// 16 bits, and s < Z <= 1024).  ent ends with kQcEntPad zero words, so that the kernel
// may load a whole register row (up to 16 words) from any eb_r without a bound: what lies past the row's degree is
// another row's entries or zeros, either way a column of the code, and the
// kernel reads it and drops the value.
constexpr int kQcEntPad = 16;
struct QcTables {
  std::vector<uint32_t> rows, ent;
};
void qc_build(int mb, int nb, int Z, const int32_t *shifts, QcTables &t);

}  // namespace ldpc
