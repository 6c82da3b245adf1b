"""div_n's shared reciprocal carries div_core's 1 + 2^-40 scale in the Newton
step's residual (csrc/ldpc_exact.hpp).  div_core's sure-pass test is sound
only while every b * yk stays inside (1 + 2^-41, 1 + 2^-39) -- above 1 in
particular -- so this measures the products themselves, exactly (product and
fma residual), for div_n<1..3> on the operand families of
test_exact.py::test_batched_division_is_ieee, with the seed off by the same
amounts before the Newton step, and checks every quotient against the host's
IEEE a / b.  The header's bound is |b yk - (1 + 2^-40)| < 2^-46.9."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "div_window_check.cc")
N = 150_000  # per family (a multiple of 1, 2 and 3)


@pytest.fixture(scope="module")
def dw(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dw") / "div_window_check.so")
    flags = ["-O2", "-ffp-contract=off", "-fPIC", "-shared"]
    if "fma" in open("/proc/cpuinfo").read().split():
        flags.append("-mfma")  # speed only: every fused operation is an explicit fma
    subprocess.check_call(["g++"] + flags + ["-o", so, SRC, "-lm"])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def families():
    """(a, b) of test_batched_division_is_ieee: the three divisions of the
    sum-product pass and the hard significands; computed once, read only."""
    rng = np.random.default_rng(105)
    n = N
    hard = (np.int64(0x3FF0000000000000) |
            (rng.integers(0, 2, n) * ((1 << 52) - 1) ^ rng.integers(0, 1 << 20, n))).view(np.float64)
    cases = [(rng.uniform(-2.2, -1.8, n), rng.uniform(5, 7, n)),
             (rng.uniform(0, 0.87, n), rng.uniform(1.13, 2, n)),
             (np.full(n, 2.0), 2 + np.exp(rng.uniform(1.8, 44, n))),
             (1 + rng.uniform(-1, 1, n), 1 - rng.uniform(-1, 1, n) * 10.0 ** -rng.uniform(0, 16, n)),
             (hard, np.roll(hard, 1)), (rng.uniform(1, 2, n), hard),
             (np.ones(n), np.full(n, 1 - 2.0 ** -53)),
             (1 + rng.integers(0, 1 << 12, n) * 2.0 ** -52,
              (np.int64(0x3FEFFFFFFFFFFFFF) - rng.integers(0, 1 << 8, n)).view(np.float64)),
             (1 + rng.uniform(-1, 1, n) * 2.0 ** -53 * rng.integers(0, 3, n),
              1 - rng.integers(0, 3, n) * 2.0 ** -53)]
    out = []
    for a, b in cases:
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        a.setflags(write=False)
        b.setflags(write=False)
        out.append((a, b))
    return out


@pytest.mark.parametrize("perturb", [0, 1, -1, 3, -3, 8, -8, 1 << 20, -(1 << 22)])
def test_reciprocal_products_stay_in_window(dw, families, perturb):
    dw.set_rcp_perturb(perturb)
    try:
        lo, hi = np.inf, -np.inf
        for f, (a, b) in enumerate(families):
            for k in (1, 2, 3):
                out = np.zeros(2, np.int64)
                ext = np.zeros(2, np.float64)
                dw.check_window(ctypes.c_int(k), a.ctypes.data_as(ctypes.c_void_p),
                                b.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(a.size),
                                out.ctypes.data_as(ctypes.c_void_p),
                                ext.ctypes.data_as(ctypes.c_void_p))
                lo, hi = min(lo, ext[0]), max(hi, ext[1])
                assert out[0] == 0, ("b*yk outside (1+2^-41, 1+2^-39)", f, k, int(out[0]),
                                     ext[0].hex(), ext[1].hex())
                assert out[1] == 0, ("quotient differs from a / b", f, k, int(out[1]))
        print("perturb %d: b*yk - 1 in [2^-40 %+.3g, 2^-40 %+.3g]"
              % (perturb, lo - 2.0 ** -40, hi - 2.0 ** -40))
    finally:
        dw.set_rcp_perturb(0)
