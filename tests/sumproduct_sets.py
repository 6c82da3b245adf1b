"""Frames for the sum-product restatement (tests/sumproduct_ref.py), shared by
its host test and the device test of the inexact precisions.

On the default H: 64 ordinary frames of the golden fixture (32 at 0 dB, 32 at
2 dB: a mix of frames that stop early and frames that run to cap 50), frames
far outside the channel's range, and frames that hold +-inf / NaN samples."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAPS = (1, 5, 50)
ETS = (1, 5)
SCALES = (8.0, 30.0, 1e3, 1e-30)
_cache = {}


def _fixture():
    if "fd" not in _cache:
        _cache["fd"] = np.load(os.path.join(GOLDEN, "frames_default.npz"))
    return _cache["fd"]


def default_h():
    return np.array(_fixture()["H_reordered"])


def default_csr():
    H = default_h()
    rows, cols = np.nonzero(H)
    rp = np.zeros(H.shape[0] + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return H.shape[0], H.shape[1], np.cumsum(rp).astype(np.int32), cols.astype(np.int32)


def _ro(y):
    y = np.ascontiguousarray(y, np.float32)
    y.setflags(write=False)
    return y


def ordinary():
    """db0_llr[0:32] and db2_llr[32:64]: by the C oracle (f64, cap 50) at least
    16 of the 64 stop before the cap and at least 4 reach it
    (tests/test_sumproduct_ref_host.py asserts it)."""
    fd = _fixture()
    return _ro(np.concatenate([fd["db0_llr"][0:32], fd["db2_llr"][32:64]]))


def extreme():
    """8 frames each scaled by 8, 30, 1e3 (tanh saturates: T = +-1, infinite
    check messages, inf - inf) and 1e-30"""
    base = _fixture()["db2_llr"][:8].astype(np.float64)
    y = np.concatenate([base * a for a in SCALES]).astype(np.float32)
    assert np.isfinite(y).all()
    return _ro(y)


def nonfinite():
    """16 frames with 1-3 samples set to +-inf or NaN, built as
    tests/test_gpu_decode.py::test_non_finite_samples builds them"""
    y = _fixture()["db2_llr"][:16].copy()
    rng = np.random.default_rng(99)
    for b in range(y.shape[0]):
        for _ in range(1 + b % 3):
            y[b, rng.integers(0, 64)] = rng.choice([np.inf, -np.inf, np.nan])
    assert (~np.isfinite(y)).any(axis=1).all()
    return _ro(y)


SETS = dict(ordinary=ordinary, extreme=extreme, nonfinite=nonfinite)


def other_code(name):
    """(H, frames) of hData1 / hData5: the golden fixture's reordered H and frames."""
    fo = np.load(os.path.join(GOLDEN, "frames_other.npz"))
    return np.array(fo[name + "_H_reordered"]), _ro(fo[name + "_llr"])


def same_posteriors(a, b):
    """float32 posteriors as bit patterns, NaN positions equal"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(out, ref, what, post="post"):
    """bits, packed, iters, synd equal and posteriors equal as bit patterns"""
    for k in ("bits", "packed", "iters", "synd"):
        if k in out:
            np.testing.assert_array_equal(out[k], ref[k], err_msg="%s: %s" % (what, k))
    if post in out:
        same = same_posteriors(out[post], ref["post"])
        assert same.all(), "%s: %d posteriors differ, first at %s: %r vs %r" % (
            what, (~same).sum(), np.argwhere(~same)[0], np.asarray(out[post])[~same][:4],
            np.asarray(ref["post"])[~same][:4])
