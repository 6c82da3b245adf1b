"""The host half of tests/test_gpu_math.py.

The device tests upload the pools of tests/math_sets.py and compare each
function of the decode kernels with glibc's values from the oracle's
elementwise helpers.  Here, without a GPU: the helpers return what the host
libm returns (the calls of tests/native/exact_check.cc); the exact forms of
ldpc_exact.hpp pass on the very pools the device gets, with an exact
reciprocal seed, so a failure on the GPU points at the device; and the
precision-3 bound check catches a tanh 8 ulp off on [8, 16]."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import math_sets as ms
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "exact_check.cc")


@pytest.fixture(scope="module")
def ec(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ecm") / "exact_check.so")
    flags = ["-O2", "-ffp-contract=off", "-fPIC", "-shared"]
    if "fma" in open("/proc/cpuinfo").read().split():
        flags.append("-mfma")  # speed only: every fused operation is an explicit fma
    subprocess.check_call(["g++"] + flags + ["-o", so, SRC, "-lm"])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _mism(fn, *arrays, k=None):
    arrays = [np.ascontiguousarray(a, np.float64) for a in arrays]
    out = np.zeros(2, np.int64)
    args = ([ctypes.c_int(k)] if k is not None else []) + [_ptr(a) for a in arrays]
    fn(*args, ctypes.c_int64(arrays[0].size), _ptr(out))
    return int(out[0]), int(out[1])


def _libm(ec, fn, a, b=None):
    a = np.ascontiguousarray(a, np.float64)
    b = a if b is None else np.ascontiguousarray(b, np.float64)
    out = np.empty_like(a)
    ec.libm_eval(ctypes.c_int(fn), _ptr(a), _ptr(b), ctypes.c_int64(a.size), _ptr(out))
    return out


def test_helpers_are_the_host_libm(ec):
    """orc_tanh_half, orc_log_ratio and orc_div against the libm calls of
    tests/native/exact_check.cc, as bit patterns, on SPECIALS and a sweep"""
    rng = np.random.default_rng(31)
    x = np.concatenate([ms.SPECIALS, rng.normal(0, 8, 50_000)])
    assert ms.same_bits(orc.tanh_half(x), _libm(ec, 0, x)).all()
    T = np.concatenate([ms.SPECIALS, rng.uniform(-1, 1, 50_000), ms.log_ratio_sets(4096)[-1]])
    assert ms.same_bits(orc.log_ratio(T), _libm(ec, 1, T)).all()
    a = np.concatenate([ms.SPECIALS, rng.normal(0, 8, 50_000)])
    b = np.concatenate([ms.SPECIALS[::-1], rng.normal(0, 8, 50_000)])
    assert ms.same_bits(orc.div(a, b), _libm(ec, 2, a, b)).all()
    with np.errstate(all="ignore"):
        assert ms.same_bits(orc.div(a, b), a / b).all()


def test_float_helpers():
    """tanhf(x / 2.0f), logf(q) and logf((1 + T) / (1 - T)) are float functions
    of float operands: results at float precision, the edges glibc defines"""
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -3.0], np.float32)
    z = orc.tanh_half_f32(x)
    assert z.dtype == np.float32
    assert ms.same_bits(z[:4], np.array([0.0, -0.0, 1.0, -1.0], np.float32)).all() and np.isnan(z[4])
    assert ms.ulps(z[5:], np.tanh(x[5:].astype(np.float64) / 2).astype(np.float32)).max() <= 1
    T = np.array([1.0, -1.0, 0.0, -0.0, 0.5], np.float32)
    e = orc.log_ratio_f32(T)
    assert e[0] == np.inf and e[1] == -np.inf and e[2] == 0 and e[3] == 0
    q = ((np.float32(1) + T[4:]) / (np.float32(1) - T[4:])).astype(np.float32)
    assert ms.same_bits(orc.log_f32(q), e[4:]).all()


def test_exact_forms_on_the_device_pools(ec):
    """no perturbation: tanh_half_n<3>, log_ratio_n<3> and div_n<1..3> equal
    glibc / IEEE division on the pools the device tests upload, and glibc's
    values there are the oracle helpers' values"""
    m = ms.triples(ms.tanh_pool())
    assert _mism(ec.check_tanh_half, m) == (0, 0)
    T = ms.triples(ms.ratio_pool())
    assert np.all(~(np.abs(T) > 1))
    assert _mism(ec.check_log_ratio, T) == (0, 0)
    a, b = ms.division_pool()
    for k in (1, 2, 3):
        assert _mism(ec.check_div, a, b, k=k) == (0, 0), k
    cold = ms.whole_wave_cold()
    for name in ("near1", "zeros", "edge"):
        assert _mism(ec.check_log_ratio, cold[name]) == (0, 0), name
    for k in (1, 2, 3):
        assert _mism(ec.check_div, *cold["flagged"], k=k) == (0, 0), k
    mm, mask = ms.masked_operands(m)
    assert (mm[mask != 0] == 0).all() and mask.sum() > 1000
    assert _mism(ec.check_tanh_half, mm) == (0, 0)


def test_whole_wave_sets_are_cold():
    cold = ms.whole_wave_cold()
    T = cold["near1"]
    q = (1 + T) / (1 - T)
    assert T.size == 4 * ms.WAVE and np.all(np.abs(q - 1) < 1 / 16) and np.all(q != 1)
    assert np.all(cold["zeros"] == 0) and np.signbit(cold["zeros"]).sum() == 2 * ms.WAVE
    assert np.all(~(np.abs(cold["edge"]) < 1))


def test_the_three_ulp_check_can_fail():
    """glibc's own values pass precision 3's tanh bounds; the same values 8 ulp
    off for |m| in [8, 16] do not"""
    m = ms.fast_tanh_pool()
    ref = orc.tanh_half(m)
    assert ms.assert_fast_tanh(m, ref.copy(), ref) == (0, 0, 0)
    off = ref.copy()
    sel = (np.abs(m) >= 8) & (np.abs(m) <= 16)
    assert sel.sum() > 1000
    off[sel] = (off[sel].view(np.int64) - 8).view(np.float64)
    assert ms.ulps(off, ref).max() == 8
    with pytest.raises(AssertionError):
        ms.assert_fast_tanh(m, off, ref)
