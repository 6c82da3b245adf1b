"""The quasi-cyclic codes the encoder tests share (tests/test_qc_encode_host.py,
tests/test_gpu_qc_encode.py, tests/native/qc_encode_driver.cc).  All base
matrices are synthetic: codes.qc_parity_core's seeded draws, next to the
lower-triangular ones of tests/qc_cases.py.

Run as a script it writes every case with five data rows as text for the
native driver: per case "mb nb Z B", the mb * nb shifts, then B rows of K bits."""
import numpy as np

import qc_cases

INFO_DEG = 3

# name -> (mc, me, nb, Z), (a, b, x), seed, frames on the GPU
CORE = {
    "W27": ((12, 0, 24, 27), (1, 0, 6), 21, 37),     # Z below a wave, 802.11n shape
    "W96": ((12, 0, 24, 96), (95, 0, 5), 22, 16),    # 1.5 waves, shift Z - 1 wraps
    "W7": ((4, 0, 10, 7), (0, 1, 2), 23, 64),        # b != 0 (BG2-core shape), odd Z
    "W3": ((3, 0, 6, 5), (2, 4, 1), 24, 5),          # the smallest core
    "X16": ((4, 6, 18, 16), (1, 0, 1), 25, 33),      # core + extension, rotated diagonals
    "X384": ((4, 3, 12, 384), (1, 0, 2), 26, 8),     # six waves, level wider than the block
    "X64": ((4, 3, 12, 64), (1, 0, 2), 27, 5),       # (host only)
    "E9": ((0, 5, 12, 9), (1, 0, None), 28, 5),      # extension alone, rotated diagonals (host only)
}
GPU_CORE = ("W27", "W96", "W7", "W3", "X16", "X384")
TRIANGULAR = tuple("ABCDEFG")          # tests/qc_cases.py, core 0
T24K = (4, 24, 1024, 3, 7)             # qc_dual_diagonal: N = 24 576


def base_of(name):
    """(base, Z, core) of a case."""
    from ldpc_ece535a import codes
    if name in CORE:
        (mc, me, nb, Z), (a, b, x), seed, _ = CORE[name]
        return codes.qc_parity_core(mc, me, nb, Z, INFO_DEG, seed, a=a, b=b, x=x), Z, mc
    if name == "L0":    # X16 without the information entries of a core and an extension row
        base, Z, mc = base_of("X16")
        base[1, 10:] = -1
        base[6, 10:] = -1
        return base, Z, mc
    if name == "T24k":
        return codes.qc_dual_diagonal(*T24K), T24K[2], 0
    if name == "T68k":      # N = 69 632: a frame past 64 KiB of LDS
        return codes.qc_dual_diagonal(8, 68, 1024, 2, 31), 1024, 0
    if name == "T168k":     # N = 172 032: a frame past a workgroup's LDS
        return codes.qc_dual_diagonal(8, 168, 1024, 1, 32), 1024, 0
    if name == "b39":
        return qc_cases.boundary_base(39), 384, 0
    base, Z = qc_cases.base_of(name)
    return base, Z, 0


HOST_CASES = TRIANGULAR + ("b39",) + tuple(CORE) + ("L0",)


def data_of(name, B):
    """B seeded rows of information bits for a case."""
    base, Z, _ = base_of(name)
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name)) + 1000))
    return rng.integers(0, 2, (B, (base.shape[1] - base.shape[0]) * Z), np.uint8)


def refusals():
    """name -> (base, Z, block row, block column): one edit each of an
    encodable base matrix that breaks the form at that cell."""
    out = {}
    w, Z, mc = base_of("W27")
    t = w.copy()
    t[mc - 1, 0] = 2                     # bottom shift 2, top shift 1
    out["bottom_differs"] = (t, Z, mc - 1, 0)
    t = w.copy()
    t[8, 0] = 3                          # x = 6 already there
    out["fourth_entry"] = (t, Z, 8, 0)
    t = w.copy()
    t[4, 5] = 1                          # above the diagonal of the dual pair
    out["dual_shift_upper"] = (t, Z, 4, 5)
    t = w.copy()
    t[5, 5] = 1
    out["dual_shift_diagonal"] = (t, Z, 5, 5)
    x, Z, mc = base_of("X16")
    t = x.copy()
    t[6, 8] = 0
    out["right_of_diagonal"] = (t, Z, 6, 8)
    t = x.copy()
    t[7, 7] = -1
    out["missing_diagonal"] = (t, Z, 7, 7)
    a, Z = qc_cases.base_of("A")
    t = a.copy()
    t[3, 3] = -1
    out["missing_diagonal_triangular"] = (t, Z, 3, 3)
    return out


def main():
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd"))
    for name in HOST_CASES:
        base, Z, _ = base_of(name)
        d = data_of(name, 5)
        print(base.shape[0], base.shape[1], Z, d.shape[0])
        print(" ".join(str(int(v)) for v in base.reshape(-1)))
        for row in d:
            print("".join(str(int(v)) for v in row))


if __name__ == "__main__":
    main()
