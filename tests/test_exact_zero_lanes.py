"""The column-centric loop's forms of ldpc_exact.hpp on the host.

tanh_half_n's masked overload takes, per value, the flag "this operand is a
structural +-0" instead of comparing the operand with zero.  It must return
host libm's tanh(m / 2) bit for bit whatever the flags say about the zeros:
no flag set, flags exactly on the zeros, and flags on none of the zeros (every
+-0 then takes the cold x (1 + x) path) while set on every in-range operand.
The operand sets are test_exact.py's (the same generators), with zeros mixed
into ordinary triples besides.

The rewritten helpers (expm1_n's one-offset table lookups, log_near1_lean,
fma3_) are held to the functions they replace on the same sets and on +-64
ulp around every class boundary."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "zero_lanes_check.cc")
LN2 = np.log(2.0)


@pytest.fixture(scope="module")
def zc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("zc") / "zero_lanes_check.so")
    flags = ["-O2", "-ffp-contract=off", "-fPIC", "-shared"]
    if "fma" in open("/proc/cpuinfo").read().split():
        flags.append("-mfma")  # speed only: every fused operation is an explicit fma
    subprocess.check_call(["g++"] + flags + ["-o", so, SRC, "-lm"])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _call(fn, *arrays, mode=None, nout=2):
    arrays = [np.ascontiguousarray(a, np.float64) for a in arrays]
    n = min(a.size for a in arrays)
    out = np.zeros(nout, np.int64)
    args = ([ctypes.c_int(mode)] if mode is not None else []) + [_ptr(a) for a in arrays]
    fn(*args, ctypes.c_int64(n), _ptr(out))
    return [int(x) for x in out]


def _triples(x):
    x = np.asarray(x, np.float64).ravel()
    pad = (-x.size) % 3
    return np.concatenate([x, np.full(pad, 0.5)]) if pad else x


def _around(points, width=64):
    """every double within `width` ulp of each point, both signs"""
    pts = np.asarray(points, np.float64)
    b = pts.view(np.int64)[:, None] + np.arange(-width, width + 1)[None, :]
    v = b.view(np.float64).ravel()
    return np.concatenate([v, -v])


# class boundaries of tanh(m / 2): expm1's k classes switch at |u| = 0.5 ln2,
# 1.5 ln2 (high word) and (k + 1/2) ln2; tanh's at |m| = 2, 44, 2^-54; the
# masked form's own range test at 2^-54 and 13.5
EDGES = ([0.5 * LN2, 1.5 * LN2, 2.0, 44.0, 2.0 ** -54, 2.0 ** -53, 13.5]
         + [(k + 0.5) * LN2 for k in range(2, 64)]
         + [float.fromhex("0x1.62e42p-2"), float.fromhex("0x1.0a2b2p0")])


@pytest.fixture(scope="module")
def tanh_sets():
    """test_exact.py::test_tanh_half_bit_identical's operands, plus zeros
    mixed into ordinary triples (a wave's lanes hold both) and +-64 ulp around
    each class boundary"""
    rng = np.random.default_rng(102)
    sets = [rng.uniform(-4, 4, 6_000_000), rng.uniform(-60, 60, 6_000_000),
            rng.normal(0, 12, 6_000_000),
            rng.uniform(-1, 1, 3_000_000) * 10.0 ** rng.uniform(-30, 0, 3_000_000),
            _around(EDGES, 512),
            np.concatenate([v := rng.integers(0x3FD62E42FEFA39EF, 0x3FD62E4300000000, 200_000,
                                               dtype=np.int64).view(np.float64), -v]),
            np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, 1e300,
                      -1e300, 2.0, -2.0, 44.0, -44.0])]
    mixed = rng.normal(0, 6, 600_000)
    mixed[rng.integers(0, mixed.size, 100_000)] = 0.0
    mixed[rng.integers(0, mixed.size, 100_000)] = -0.0
    mixed[rng.integers(0, mixed.size, 1_000)] = np.inf
    mixed[rng.integers(0, mixed.size, 1_000)] = np.nan
    mixed[rng.integers(0, mixed.size, 1_000)] = 1e-20
    sets += [mixed, _around(EDGES, 64), np.array([0.0, -0.0, 0.0, -0.0, 1.0, 0.0, 30.0, -0.0, np.nan])]
    return [_triples(s) for s in sets]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_flag", "flags_on_zeros", "zeros_unflagged"])
def test_masked_tanh_half_bit_identical(zc, tanh_sets, mode):
    for m in tanh_sets:
        mism, maxu, mism0, maxu0 = _call(zc.check_tanh_masked, m, mode=mode, nout=4)
        assert mism == 0, ("vs libm", mism, maxu)
        assert mism0 == 0, ("vs the unmasked tanh_half_n", mism0, maxu0)


def test_expm1_lean_equals_expm1(zc):
    """expm1_n<n, true> against expm1_n<n, false> on test_exact.py's expm1
    operands and around every k boundary inside its domain"""
    rng = np.random.default_rng(103)
    sets = [-rng.uniform(0, 2, 3_000_000), rng.uniform(2, 44, 3_000_000),
            -10.0 ** rng.uniform(-16, 0.3, 3_000_000), _around(EDGES, 64)]
    for u in sets:
        u = u[((u < 0) & (u > -2) & (u <= -2.0 ** -54)) | ((u >= 2) & (u < 44))]
        mism, maxu = _call(zc.check_expm1_lean, _triples(u))
        assert mism == 0, (mism, maxu)


def test_log_near1_lean_equals_log_near1(zc):
    """on the |x - 1| < 1/16 window: test_exact.py's near-1 sets, both ends of
    the window and 1.0 itself, +-64 ulp (and wider)"""
    rng = np.random.default_rng(101)
    lo, hi = 1 - 2.0 ** -4, 1 + float.fromhex("0x1.09p-4")
    sets = [1 + rng.uniform(-0.07, 0.07, 4_000_000),
            1 + rng.uniform(-1, 1, 2_000_000) * 10.0 ** rng.uniform(-17, -1, 2_000_000),
            _around([lo, hi, 1.0], 4096), _around([lo, hi, 1.0], 64)]
    for x in sets:
        x = x[(x >= lo) & (x < hi)]
        mism, maxu = _call(zc.check_log_near1_lean, x)
        assert mism == 0, (mism, maxu)


def test_fma3_is_fma(zc):
    rng = np.random.default_rng(106)
    n = 1_000_000
    s = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-8, 8, n)
    a = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-8, 8, n)
    c = -s * a * (1 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-17, 0, n))  # cancellation
    assert _call(zc.check_fma3, s, a, c)[0] == 0
