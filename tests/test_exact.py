"""ldpc_exact.hpp -- the arithmetic of the default sum-product mode -- on the
host, against the host libm (glibc: what the reference and the oracle call).

The claim is bit-identity, not closeness: tanh(m/2), expm1, log and
log((1+T)/(1-T)) must return the same double as glibc for every operand the
decoder can produce, and the batched divisions the same double as IEEE
division -- also when the shared reciprocal is off by several ulp (the GPU's
v_rcp_f64 is an approximation; its seed is refined before use).  Each test
sweeps millions of random operands plus the boundaries of every branch of
glibc's code (the k classes of expm1, tanh's |x| = 1 / 22 / 2^-55 switches,
log's |x - 1| < 1/16 window and table subintervals)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import math_sets
from math_sets import triples as _triples

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "exact_check.cc")


@pytest.fixture(scope="module")
def ec(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ec") / "exact_check.so")
    flags = ["-O2", "-ffp-contract=off", "-fPIC", "-shared"]
    if "fma" in open("/proc/cpuinfo").read().split():
        flags.append("-mfma")  # speed only: every fused operation is an explicit fma
    subprocess.check_call(["g++"] + flags + ["-o", so, SRC, "-lm"])
    lib = ctypes.CDLL(so)
    lib.self_check.restype = ctypes.c_int64
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _call(fn, *arrays, mode=None):
    arrays = [np.ascontiguousarray(a, np.float64) for a in arrays]
    n = min(a.size for a in arrays)
    out = np.zeros(2, np.int64)
    args = ([ctypes.c_int(mode)] if mode is not None else []) + [_ptr(a) for a in arrays]
    fn(*args, ctypes.c_int64(n), _ptr(out))
    return int(out[0]), int(out[1])


def test_constants_match_host_libm(ec):
    """ldpc_glibc_log.hpp holds this libm's __log_data (regenerate with
    tools/gen_glibc_log.py if the image's glibc changes)."""
    assert ec.self_check() == 0
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_glibc_log.py"), "--check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_log_bit_identical(ec):
    sets = math_sets.log_sets()
    for x in sets:
        mism, maxu = _call(ec.check_log, x, mode=0)
        assert mism == 0, (mism, maxu)
    # the decoder's form on its own domain: normal [2^-60, 2^60] (log_ratio_n
    # handles T = +-1 / NaN, i.e. ratios 0 / inf / NaN, itself)
    for x in sets[:4] + [np.array([2.0 ** -60, 2.0 ** 60, 1.0])]:
        x = x[(x >= 2.0 ** -60) & (x <= 2.0 ** 60)]
        assert _call(ec.check_log, x, mode=1)[0] == 0


def test_tanh_half_bit_identical(ec):
    sets = math_sets.tanh_half_sets()
    for m in sets:
        mism, maxu = _call(ec.check_tanh_half, _triples(m))
        assert mism == 0, (mism, maxu)


def test_expm1_bit_identical(ec):
    for u in math_sets.expm1_sets():
        mism, maxu = _call(ec.check_expm1, _triples(u))
        assert mism == 0, (mism, maxu)


def test_log_ratio_bit_identical(ec):
    sets = math_sets.log_ratio_sets()
    for T in sets:
        mism, maxu = _call(ec.check_log_ratio, _triples(T))
        assert mism == 0, (mism, maxu)


@pytest.mark.parametrize("perturb", [0, 1, -1, 3, -3, 8, -8, 1 << 20, -(1 << 22)])
def test_batched_division_is_ieee(ec, perturb):
    """div_n<k> for k = 1..3 equals a / b with the shared reciprocal seed off
    by `perturb` ulp (up to 2^22): the residual correction and the exact
    residual test make the result independent of the seed's last bits.  Operands: the
    three divisions of the sum-product pass (expm1's (r1 - t) / (6 - x t) ~
    O(1), tanh's -t/(t+2) or 2/(t+2), (1+T)/(1-T) down to 2^-53) and
    significands with long runs of ones / zeros (the hard cases of division)."""
    ec.set_rcp_perturb(perturb)
    try:
        cases = math_sets.division_cases(perturb)
        for a, b in cases:
            for k in (1, 2, 3):
                mism, maxu = _call(lambda *args: ec.check_div(ctypes.c_int(k), *args), a, b)
                assert mism == 0, (k, mism, maxu)
    finally:
        ec.set_rcp_perturb(0)
