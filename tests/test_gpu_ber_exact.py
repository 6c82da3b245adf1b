"""GPU: ber.sweep equals the oracle run on the same samples.

A point of the sweep is a function of (seed, index, Eb/N0) alone:

    s0      = (seed * 1000003 + i) & 0xFFFFFFFF
    data    = ldpc_random_bits(B * K, s0)
    cw      = encode(data)
    samples = ldpc_bpsk_awgn(cw, B * N, sigma_of(Eb/N0), s0 ^ 0x5DEECE66D)
    ber     = mean over frames of (bits in error / N),  fer = frames with synd > 0

The test derives the seeds itself, takes the data from tests/channel_ref.py
and the codewords from the host encoder, makes the samples with one call of
the device channel (deterministic, and held to its restatement by
tests/test_gpu_channel.py), decodes them with the C oracle (methods 0 to 3)
and tests/layered_ref.py, and forms ber and fer as above.  Every curve of the
sweep must equal those: fer as integers, ber as the same float64 expression.
So a stale output buffer carried from one decoder to the next, a division by
K, two points on one noise seed or fer from the wrong array all show."""
import numpy as np
import pytest

import channel_ref as cr
import layered_ref as lref

pytestmark = pytest.mark.gpu

GRID = [0.0, 3.0, 6.0]
ITERS = 5
SCALE = 0.8125


@pytest.fixture(scope="module")
def dec():
    import ldpc_ece535a as L
    d = L.Decoder()
    assert (d.M, d.N) == (32, 64)
    return d


def point_seeds(seed, i):
    s0 = (int(seed) * 1000003 + i) & 0xFFFFFFFF
    return s0, s0 ^ 0x5DEECE66D


def point_samples(dec, seed, i, db, B):
    """(codewords, samples) of point i."""
    import torch
    import ldpc_ece535a as L
    from ldpc_ece535a import _capi, ber
    s0, s1 = point_seeds(seed, i)
    data = cr.random_bits(B * dec.K, s0).reshape(B, dec.K)
    cw = L.encode(dec.H, data)
    d_cw = torch.from_numpy(cw).cuda(0)
    d_tx = torch.empty((B, dec.N), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    _capi.bpsk_awgn(d_cw.data_ptr(), B * dec.N, ber.sigma_of(db), s1, d_tx.data_ptr())
    torch.cuda.synchronize()
    return cw, d_tx.cpu().numpy()


def figures(cw, out):
    N = cw.shape[1]
    err = (out["bits"] != cw).sum(axis=1).astype(np.float64)
    return float((err / N).mean()), int((out["synd"] > 0).sum())


_expected = {}


def expected(dec, seed, B, layered):
    """The curves of a sweep over GRID, computed once per (seed, B, layered)."""
    key = (seed, B, layered)
    if key not in _expected:
        _expected[key] = _compute(dec, seed, B, layered)
    return _expected[key]


def _compute(dec, seed, B, layered):
    from oracle import oracle as orc
    from ldpc_ece535a import ber
    csr = (dec.M, dec.N, dec.row_ptr, dec.col_idx)
    names = [name for name, _ in ber.METHODS] + ([ber.LAYERED] if layered else [])
    want = {name: {"ber": [], "fer": []} for name in names}
    for i, db in enumerate(GRID):
        cw, y = point_samples(dec, seed, i, db, B)
        for name, m in ber.METHODS:
            b, f = figures(cw, orc.decode_batch(m, dec.H, y, ITERS))
            want[name]["ber"].append(b)
            want[name]["fer"].append(f)
        if layered:
            b, f = figures(cw, lref.decode(csr, dec.layers, y, ITERS, scale=SCALE, precision=0))
            want[ber.LAYERED]["ber"].append(b)
            want[ber.LAYERED]["fer"].append(f)
    return want


def test_seed_derivation_separates_the_points():
    """No two points of the two sweeps share a data or a noise seed, and no
    noise seed is a data seed."""
    seeds = [point_seeds(s, i) for s in (0, 7) for i in range(len(GRID))]
    flat = [v for pair in seeds for v in pair]
    assert len(set(flat)) == len(flat)
    assert point_seeds(7, 2) == (7000023, 7000023 ^ 0x5DEECE66D)


@pytest.mark.parametrize("seed", [0, 7])
def test_sweep_equals_oracle(dec, seed):
    from ldpc_ece535a import _capi, ber
    assert [m for _, m in ber.METHODS] == [_capi.METHOD_HARD, _capi.METHOD_BITFLIP,
                                           _capi.METHOD_LOGDOMAIN, _capi.METHOD_SUMPRODUCT]
    want = expected(dec, seed, 64, layered=True)
    got = ber.sweep(dec, GRID, frames=64, iterations=ITERS, seed=seed, precision=0,
                    layered_scale=SCALE)
    assert list(got) == list(want)
    for name in want:
        assert got[name]["fer"] == want[name]["fer"], name
        assert got[name]["ber"] == want[name]["ber"], name
        assert all(type(f) is int for f in got[name]["fer"])
    # the settings show what they are meant to: the curves differ from each other and
    # along the grid, and frames fail (a sweep without errors would equal anything).
    # BitFlip is the exception: the reference flips a bit on more than M / 2 = 16 votes,
    # no column of this H has more than 4, so its decision is the hard one
    assert want["BitFlip"] == want["BPSK"]
    curves = [tuple(want[n]["ber"]) for n in want if n != "BitFlip"]
    assert len(set(curves)) == len(curves) == 4
    for n in want:
        assert want[n]["ber"][0] > want[n]["ber"][2] and want[n]["fer"][0] > 0
    four = ber.sweep(dec, GRID, frames=64, iterations=ITERS, seed=seed, precision=0)
    assert list(four) == [n for n, _ in ber.METHODS]
    for name in four:
        assert four[name] == {k: want[name][k] for k in ("ber", "fer")}, name


def test_the_points_of_a_sweep_differ_by_seed(dec):
    """Seeds 0 and 7 give different figures: the seed reaches the draws."""
    a, b = (expected(dec, s, 64, layered=False) for s in (0, 7))
    assert all(a[n]["ber"] != b[n]["ber"] for n in a)


def test_one_frame(dec):
    from ldpc_ece535a import ber
    want = expected(dec, 7, 1, layered=True)
    got = ber.sweep(dec, GRID, frames=1, iterations=ITERS, seed=7, precision=0,
                    layered_scale=SCALE)
    for name in want:
        assert got[name] == want[name], name
        assert all(f in (0, 1) for f in got[name]["fer"])


def test_no_frames(dec):
    from ldpc_ece535a import ber
    got = ber.sweep(dec, GRID, frames=0, iterations=ITERS, seed=7, precision=0,
                    layered_scale=SCALE)
    assert list(got) == [n for n, _ in ber.METHODS] + [ber.LAYERED]
    for name in got:
        assert got[name] == {"ber": [0.0] * 3, "fer": [0] * 3}, name
