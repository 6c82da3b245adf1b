"""The codes the large-code host test shares with its native driver
(tests/test_large_code_host.py, tests/native/large_code_driver.cc): the
reference's own H after reorderHMatrix (32 x 64, the identity order is the only
one), a rate-3/4 IRA code in the DVB-S2 style (M = 1800, a multiple of 360, rows
of up to 14 edges: both orders, 16-slot descriptors) and a quasi-cyclic code
whose M = 500 is no multiple of 360 or of the kernels' 256-item blocks and
whose Z = 100 circulants give a wave's edges up to four runs (the first two
codes have waves with more, which keep explicit lists).

Run as a program it writes the cases the driver reads, per case "M N E", the
M + 1 row offsets, the E columns:
    python tests/large_code_cases.py | gr-ldpc_ece535a_amd/lib/large_code_asan
"""
import numpy as np

NAMES = ("reference", "ira_dc14", "qc_m500")
FORCE = (None, "0", "1")     # LDPC_MSN_ORDER as the driver sets it, in its order


def csr_of(name):
    from ldpc_ece535a import _capi, codes
    if name == "reference":
        Hr, _ = _capi.reorder_h(_capi.default_h())
        rows, cols = np.nonzero(Hr)      # row-major, columns ascending
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=Hr.shape[0]))])
        return Hr.shape[0], Hr.shape[1], rp.astype(np.int32), cols.astype(np.int32)
    if name == "ira_dc14":
        return codes.ira_from_table(
            codes.dvbs2_like_table(3, K=5400, N=7200, hi_groups=3, hi_deg=8, lo_deg=3), 5400, 7200)
    if name == "qc_m500":
        return codes.qc_expand(codes.qc_dual_diagonal(5, 12, 100, 3, 7), 100)
    raise KeyError(name)


def text():
    """The cases as the driver reads them."""
    out = []
    for name in NAMES:
        M, N, rp, ci = csr_of(name)
        out.append("%d %d %d\n%s\n%s\n" % (M, N, len(ci), " ".join(str(int(v)) for v in rp),
                                           " ".join(str(int(v)) for v in ci)))
    return "".join(out)


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd"))
    sys.stdout.write(text())
