"""tests/sumproduct_ref.py on the host.

With glibc's tanh(m / 2) and log((1 + T) / (1 - T)) (the oracle's elementwise
helpers) at float64 the numpy restatement is the C oracle's sum-product bit
for bit: decisions, packed bytes, iteration counts, syndrome weights and
posteriors, on four codes, at caps 1, 5 and 50 and et_period 1 and 5, on
ordinary, extreme and non-finite frames.  That is what lets the device test
(tests/test_gpu_sumproduct_inexact.py) plug the device's two functions into
it and call the result the contract of precisions 1 and 3.

At float32, with the host's tanhf / logf, it is a different decoder from the
double one on every frame (the float path is not silently double), and it
tells a reversed row product and a column sum started from r apart from the
reference's order: the mutations a device test built on it must catch."""
import numpy as np
import pytest

import shape_cases as sc
import sumproduct_ref as spr
import sumproduct_sets as ss
from oracle import oracle as orc

LARGE_CASE = "u_48x96"   # the smallest large-code case (fewest edges)

GLIBC = dict(tanh_half=orc.tanh_half, check_msg=orc.log_ratio, Real=np.float64)
HOST32 = dict(tanh_half=orc.tanh_half_f32, check_msg=orc.log_ratio_f32, Real=np.float32)


def _csr(H):
    M, N = H.shape
    return (M, N) + sc.dense_to_csr(H)


def _codes():
    yield "default", ss.default_h(), np.concatenate([ss.ordinary(), ss.extreme(), ss.nonfinite()])
    for name in ("hData1", "hData5"):
        H, y = ss.other_code(name)
        yield name, H, y
    c = sc.CASES[LARGE_CASE]
    yield LARGE_CASE, np.array(c.H), c.frames[:32]


def test_the_frames_hold_the_cases():
    """by the C oracle alone: of the 64 ordinary frames at least 16 stop before
    cap 50 and at least 4 reach it; the extreme frames produce non-finite
    posteriors from finite samples"""
    ref = orc.decode_batch(1, ss.default_h(), ss.ordinary(), 50)
    assert (ref["iters"] < 50).sum() >= 16 and (ref["iters"] == 50).sum() >= 4
    ext = orc.decode_batch(1, ss.default_h(), ss.extreme(), 50, want_post=True)
    assert not np.isfinite(ext["post"]).all()
    assert sc.LARGE and min(sc.LARGE, key=lambda n: int(sc.CASES[n].H.sum())) == LARGE_CASE


@pytest.mark.parametrize("et", ss.ETS)
@pytest.mark.parametrize("cap", ss.CAPS)
def test_equals_the_c_oracle_at_float64(cap, et):
    for name, H, y in _codes():
        ref = orc.decode_batch(1, H, y, cap, want_post=True, et_period=et, nthreads=sc.threads())
        out = spr.decode(_csr(H), y, cap, et_period=et, **GLIBC)
        ss.assert_same(out, ref, "%s cap %d et_period %d" % (name, cap, et))
        # the posteriors as doubles round to the oracle's floats, so they are its doubles' floats
        assert out["post_real"].dtype == np.float64


def test_negative_polarity():
    y = ss.ordinary()
    ref = orc.decode_batch(1, ss.default_h(), y, 5, want_post=True, polarity=-1.0)
    out = spr.decode(ss.default_csr(), y, 5, polarity=-1.0, **GLIBC)
    ss.assert_same(out, ref, "polarity -1")


def test_float32_is_not_double():
    """with the host's float functions at float32 every frame's posteriors
    differ from the double oracle's"""
    y = np.concatenate([ss.ordinary(), ss.extreme()[:8]])
    ref = orc.decode_batch(1, ss.default_h(), y, 5, want_post=True)
    out = spr.decode(ss.default_csr(), y, 5, **HOST32)
    assert out["post_real"].dtype == np.float32
    differ = ~ss.same_posteriors(out["post"], ref["post"])
    assert differ.any(axis=1).all(), np.flatnonzero(~differ.any(axis=1))


@pytest.mark.parametrize("mutation", ["reverse_product", "sum_from_r"])
def test_float32_tells_the_mutations_apart(mutation):
    """the host-callable restatement at float32 against itself: a row product
    taken in reverse order, and a column sum started from r instead of 0,
    change posteriors on the ordinary frames at cap 5"""
    y = ss.ordinary()
    ref = spr.decode(ss.default_csr(), y, 5, **HOST32)
    out = spr.decode(ss.default_csr(), y, 5, **HOST32, **{mutation: True})
    with pytest.raises(AssertionError):
        ss.assert_same(out, ref, mutation)
    differ = ~ss.same_posteriors(out["post"], ref["post"])
    assert differ.any(axis=1).sum() >= 32, differ.any(axis=1).sum()
