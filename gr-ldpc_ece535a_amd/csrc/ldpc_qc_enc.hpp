// ldpc_qc_enc.hpp -- systematic encoding of quasi-cyclic codes whose parity
// part is dual-diagonal: recognising the form, and compiling it to a small
// step program that a host executor (here) and the device encoder
// (ldpc_aux.hip k_encode_qc) both interpret.  Host only, no device needed.
//
// Conventions (ldpc_qc.hpp): codeword = [parity (M) | data (K)], parity block
// columns 0..mb-1, information block columns mb..nb-1; for a block v of Z
// bits rot(v, s)[i] = v[(i + s) mod Z], so base entry (r, c) = s >= 0 adds
// rot(v_c, s) to the checks of block row r.  P = shifts[:, :mb].
//
// Encodable: for a core size mc (0, or 3 <= mc <= mb)
//   extension, block rows mc..mb-1: P[r, r] >= 0 (any shift), nothing right of
//     it, and block rows 0..mc-1 hold nothing in block columns mc..mb-1;
//   core (802.11n / 802.16e / 5G-NR shape): block column k, 1 <= k < mc, holds
//     exactly P[k-1, k] = P[k, k] = 0 inside the core, and block column 0
//     exactly P[0, 0] = P[mc-1, 0] = a and P[x, 0] = b for one 0 < x < mc-1.
//   Core columns are free in the extension rows.  mc = 0 is the block lower
//   triangular form.
//
// With lam_r the information part of block row r (the XOR of rot(d_c, s) over
// its entries in block columns >= mb):
//   rot(p_0, b) = lam_0 ^ ... ^ lam_{mc-1}         (everything else cancels)
//   p_k = rot(p_0, a) ^ lam_0 ^ ... ^ lam_{k-1}, ^ rot(p_0, b) when k > x
//   rot(p_r, P[r, r]) = lam_r ^ XOR over c < r of rot(p_c, P[r, c]),  r >= mc
// In both forms the parity part is invertible, so the codeword is unique.
//
// The program works on blocks of Z bytes (one bit each): block c < nb is block
// column c of the codeword, blocks nb..nb+scratch-1 are scratch (lam_r of the
// core's rows).  A step computes one block,
//   dst[(i + dst_shift) mod Z] = XOR over its sources of src[(i + shift) mod Z]
// for i in [0, Z); a source may be the destination itself at dst_shift (the
// same byte: an extension row adds the parity terms to the lam_r that level 0
// left there).  Steps are grouped in dependency levels: the steps of a level
// write distinct blocks and read, the destination aside, blocks that earlier
// levels finished.  Level 0 holds every lam_r (an extension row's goes
// straight into its parity block, already rotated), then p_0, then p_1 ..
// p_{mc-1} (the recurrence unrolled, so they share a level), then each
// extension row one level after the last parity block it reads.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace ldpc {

constexpr int64_t kQcEncLdsLimit = 163840;  // a workgroup's LDS
constexpr int kQcEncMaxWaves = 16;          // 1024 threads

struct QcEncSrc {
  int32_t block, shift;
};
struct QcEncStep {
  int32_t dst, dst_shift;
  int32_t src_begin, src_count;  // into srcs
};
struct QcEncProgram {
  int mb = 0, nb = 0, Z = 0;
  int core = 0;     // mc
  int scratch = 0;  // blocks behind the codeword's nb
  std::vector<int32_t> level_begin;  // levels + 1 entries, into steps
  std::vector<QcEncStep> steps;
  std::vector<QcEncSrc> srcs;
  int levels() const { return (int)level_begin.size() - 1; }
  // what the device encoder's workgroup declares: the codeword and the scratch
  // blocks, rounded up to 16 bytes
  int64_t lds_bytes() const { return (((int64_t)(nb + scratch) * Z + 15) / 16) * 16; }
  // its threads: a wave per 64 positions of a step, as many as the widest
  // level has, no more than that level's positions fill, at most kQcEncMaxWaves
  int threads() const;
};

// Recognises the form of a checked description (qc_check) and compiles it.
// False with the reason in *why, naming the block row and block column that
// broke the form.
bool qc_enc_compile(int mb, int nb, int Z, const int32_t *shifts, QcEncProgram &p,
                    std::string *why);

// The host executor: data B x K bytes (bit 0 counts) -> cw B x N bytes 0/1.
void qc_enc_run(const QcEncProgram &p, const uint8_t *data, int B, uint8_t *cw);

// The kernel's table, one array of words (needs lds_bytes() <= kQcEncLdsLimit,
// so that a block's byte offset fits 20 bits):
//   tab[0] = levels L, tab[1] = first step word S0 = 2 + 2 L
//   tab[2 + 2 l], tab[3 + 2 l]       level l: its first step and step count
//   tab[S0 + 3 s .. + 2]             step s: dst word, first source word, sources
//   a block word = block * Z | shift << 20
void qc_enc_pack(const QcEncProgram &p, std::vector<uint32_t> &tab);

}  // namespace ldpc
