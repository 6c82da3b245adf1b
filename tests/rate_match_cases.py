"""The rate-matching patterns the tests share (tests/test_rate_match_host.py,
tests/test_gpu_rate_match.py), on the synthetic codes of tests/qc_cases.py and
tests/layered_ref.py.  S = ncb - filler is the buffer without its fillers.

Run as a program it writes the cases tests/native/rate_match_driver.cc reads:
    python tests/rate_match_cases.py | gr-ldpc_ece535a_amd/lib/rate_match_asan
"""
import numpy as np

import qc_cases as qc

IRA = "ira720"   # layered_ref.ira_code(360, 720, 1): the table route, first-fit layers


def _shape(code):
    if code == IRA:
        return 360, 720
    (mb, nb, Z, _, _), _, _ = qc.TABLE[code]
    return mb * Z, nb * Z


def _case(code, punct, filler, cut, tx):
    """pattern = (punct, filler, ncb) with ncb = N - punct - cut (0 for cut = 0:
    the default spelling); tx(S) lists the transmissions."""
    M, N = _shape(code)
    ncb = N - punct - cut if cut else 0
    S = N - punct - cut - filler
    return dict(code=code, M=M, N=N, pattern=(punct, filler, ncb), S=S, tx=tx(S))


CASES = {
    # (a) the identity: every position once, in transmit order
    "a": _case("B", 0, 0, 0, lambda S: [(0, S)]),
    # (b) Z = 27: puncturing and fillers that split a circulant, one short transmission
    "b": _case("B", 54, 40, 0, lambda S: [(0, S - 81)]),
    # (c) a shortened buffer, a start near its end: a wrap and a repetition
    "c": _case("A", 128, 70, 64, lambda S: [(S - 100, S + 150)]),
    # (c3) E > 2 S: every column of the buffer gets two or three terms
    "c3": _case("A", 128, 70, 64, lambda S: [(S - 100, 2 * S + 150)]),
    # (d) three transmissions combined
    "d": _case("B", 54, 40, 27, lambda S: [(0, S // 2), (274, S // 3), (189, 200)]),
    # (d2) the same with the second start inside the fillers (offsets [230, 270))
    "d2": _case("B", 54, 40, 27, lambda S: [(0, S // 2), (250, S // 3), (189, 200)]),
    # (e) Z = 1, N = 40: fewer columns than threads
    "e": _case("E", 2, 3, 0, lambda S: [(5, S + 15)]),
    # (f) Z = 1024: columns beyond one stride of 1024 threads.  The buffer is the
    # K positions that are left of the information part and of the parity: no
    # frame can leave before the cap.  (f2) punctures one block column and can.
    "f": _case("F", 2048, 0, 0, lambda S: [(100, S - 96)]),
    "f2": _case("F", 1024, 0, 0, lambda S: [(100, S - 96)]),
    # (g) the table route, a pattern like (c).  The buffer is cut by one position
    # only: the parity part is an accumulator chain, and a row of it that holds
    # two unsent parity bits has nothing to tell either
    "g": _case(IRA, 60, 50, 1, lambda S: [(S - 90, S + 120)]),
}


def total(case):
    return sum(e for _, e in case["tx"])


def code_of(case):
    """(csr, plan, qc): the expanded code, its layer plan (block rows; first fit
    for the IRA code) and (base, Z) or None."""
    import layered_ref as ref
    if case["code"] == IRA:
        csr = ref.ira_code(360, 720, 1)
        return csr, ref.first_fit(csr), None
    from ldpc_ece535a import codes
    base, Z = qc.base_of(case["code"])
    return codes.qc_expand(base, Z), qc.block_rows(base.shape[0], Z), (base, Z)


def codewords(case, csr, B, seed):
    """B codewords whose last `filler` information bits are zero."""
    from ldpc_ece535a import codes
    M, N = case["M"], case["N"]
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, (B, N - M), np.uint8)
    if case["pattern"][1]:
        info[:, N - M - case["pattern"][1]:] = 0
    cw = codes.ira_encode(csr, info) if case["code"] == IRA else codes.qc_encode(csr, info)
    return cw.astype(np.uint8), rng


def received(case, csr, B, db, seed):
    """(cw, rx): the codewords and their noisy BPSK transmissions (B, sum E),
    each transmission with its own noise."""
    import rate_match_ref as rm
    cw, rng = codewords(case, csr, B, seed)
    cols = rm.columns(case["M"], case["N"], case["pattern"], case["tx"])
    x = 2.0 * cw[:, cols] - 1.0
    rx = x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)
    return cw, rx.astype(np.float32)


def plant_special(rx):
    """+-inf, runs of +0.0 and -0.0, and NaN, on strides of frames; in the
    repeating cases some of them are one of two or three terms of a column.  The
    NaNs are one value, and no column gets both infinities: IEEE 754 leaves to
    the adder which NaN a sum of two propagates and the sign of the one it
    makes of inf - inf.  In place."""
    n = rx.shape[1]
    rx[::7, 3 % n] = np.inf
    rx[1::5, 10 % n] = -np.inf
    rx[2::9, 20 % n] = np.nan
    rx[3::4, 4:7] = 0.0
    rx[5::8, 40 % n:40 % n + 4] = -0.0
    rx[4::11, n - 1] = np.nan
    rx[6::13, n // 2] = np.inf
    return rx


def strided(rx, pad, fill=np.float32(3.0e38)):
    """rx at a stride of sum E + pad, the gaps filled with a value no decode
    survives reading."""
    out = np.full((rx.shape[0], rx.shape[1] + pad), fill, np.float32)
    out[:, :rx.shape[1]] = rx
    return out


def main():
    rng = np.random.Generator(np.random.PCG64(7))
    for name, c in CASES.items():
        B = 3
        n = total(c)
        print(c["M"], c["N"], *c["pattern"], len(c["tx"]), B)
        print(" ".join("%d %d" % t for t in c["tx"]))
        bits = rng.integers(0, 2, (B, c["N"]), np.uint8)
        for row in bits:
            print("".join(str(v) for v in row))
        rx = plant_special(rng.standard_normal((B, n)).astype(np.float32))
        for row in rx.view(np.uint32):
            print(" ".join("%08x" % v for v in row))


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd")]
    main()
