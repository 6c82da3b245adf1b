"""The column-centric sum-product loop takes the lanes of its structural zeros
from a per-code mask (build_tables' zero lanes) instead of comparing every
bit message with zero.  A bit message that is exactly zero at a lane the mask
does not cover then goes through the cold paths of tanh_half_n, which must
return the same +-0.  Every result has to stay the oracle's, bit for bit.

Codes (all column-centric at precision 0):
  * the default H: low loop lengths (DVN = 3), three columns of degree 1;
  * low_empty: 32 x 64 with an empty column, two columns of degree 1 and
    weight 3 elsewhere -- the low form with all three kinds of lane;
  * gen_empty: 48 x 64 with an empty column, three of degree 1 and weight 4
    elsewhere -- the generic form (DVN = 4, the other register budget).
tests/shape_cases.py has no column-centric case with an empty column (z_empty
takes the edge form), so the two are built here with its generator.

Frames: 64 per code at 2 dB (the all-zero codeword).  Three frames in four get
+0.0 / -0.0 written into samples of columns of degree >= 2: two columns of one
row (each column's message to its other rows is then the sum of check messages
log((1 + 0) / (1 - 0)) = +0 and r = +-0: an exact zero where no mask bit is
set, from the first iteration on), and one or two more spread over other
columns.

Caps 1, 5, 50 and et_period 1, 5, through ldpc_decode_device in both launch
modes and a ring session; packed bytes, iterations, syndrome weights and (where
the route returns them) posteriors as bit patterns."""
import numpy as np
import pytest

import ldpc_ece535a as L
from shape_cases import random_code, same_bits, threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 64
_cache = {}


def _code(name):
    if name == "default":
        return None
    if name == "low_empty":
        return random_code(32, 64, {0: 1, 1: 2, 3: 61})
    return random_code(48, 64, {0: 1, 1: 3, 4: 60})


def _decoder(name):
    H = _code(name)
    return L.Decoder() if H is None else L.Decoder(H, reorder=False)


def _frames(name, H):
    """the code's 64 frames, built once and read only"""
    if name not in _cache:
        M, N = H.shape
        rng = np.random.Generator(np.random.PCG64(2020 + N + M))
        y = (-1.0 + np.sqrt(10 ** (-2.0 / 10)) * rng.standard_normal((B, N))).astype(np.float32)
        deg = H.sum(0)
        rows = [j for j in range(M) if (deg[H[j] != 0] >= 2).sum() >= 2]
        wide = np.flatnonzero(deg >= 2)
        assert rows and wide.size >= 8
        nz = 0
        for b in range(B):
            if b % 4 == 0:
                continue  # an ordinary frame
            j = rows[(5 * b) % len(rows)]
            pair = [c for c in np.flatnonzero(H[j]) if deg[c] >= 2][:2]
            more = wide[rng.integers(0, wide.size, 1 + b % 2)]
            for k, c in enumerate(list(pair) + list(more)):
                y[b, c] = 0.0 if (b + k) % 2 else -0.0
                nz += 1
        assert nz >= 3 * 48
        y.setflags(write=False)
        _cache[name] = y
    return _cache[name]


def _oracle(name, H, y, cap, et):
    from oracle import oracle as orc
    key = (name, cap, et)
    if key not in _cache:
        _cache[key] = orc.decode_batch(1, H, y, cap, nthreads=threads(), et_period=et,
                                       want_post=True)
    return _cache[key]


def _check(what, ref, packed, iters, synd, post=None):
    bad = np.flatnonzero((packed != ref["packed"]).any(axis=1))
    assert bad.size == 0, (what, "packed bytes differ on frames", bad[:8])
    np.testing.assert_array_equal(iters, ref["iters"], err_msg=what)
    np.testing.assert_array_equal(synd, ref["synd"], err_msg=what)
    if post is not None:
        same_bits(post, ref["post"], what)


def test_codes_are_what_the_test_needs():
    """the shapes (CPU only): column-centric, with the lanes the mask is for"""
    from shape_cases import kernel_shape
    for name, want in (("low_empty", (3, 1, 5, 3, True)), ("gen_empty", (4, 1, 7, 4, True))):
        H = _code(name)
        M, N = H.shape
        deg = H.sum(0)
        assert kernel_shape(M, N, int(H.sum()), int(H.sum(1).max()), int(deg.max())) == want, name
        assert (deg == 0).sum() == 1 and (deg == 1).sum() >= 2, name


@pytest.mark.parametrize("et", [1, 5])
@pytest.mark.parametrize("cap", [1, 5, 50])
@pytest.mark.parametrize("name", ["default", "low_empty", "gen_empty"])
def test_zero_lanes_vs_oracle(name, cap, et):
    dec = _decoder(name)
    H = np.asarray(dec.H)
    y = _frames(name, H)
    ref = _oracle(name, H, y, cap, et)
    N = H.shape[1]
    d_y = torch.from_numpy(np.array(y)).cuda()
    for mode in (L._capi.MODE_LATENCY, L._capi.MODE_THROUGHPUT):
        dec.set_launch_mode(mode)
        pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
        it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        sy = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        ll = torch.zeros((B, N), dtype=torch.float32, device="cuda")
        dec.decode_device(d_y.data_ptr(), B, pk.data_ptr(), method=1, max_iters=cap, et_period=et,
                          d_iters=it.data_ptr(), d_synd=sy.data_ptr(), d_llr=ll.data_ptr())
        dec.synchronize()
        _check("%s decode_device mode %d cap %d et %d" % (name, mode, cap, et), ref,
               pk.cpu().numpy(), it.cpu().numpy(), sy.cpu().numpy(), ll.cpu().numpy())
    dec.set_launch_mode(L._capi.MODE_LATENCY)
    rpk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
    rit = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rsy = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.ring_begin(method=1, max_iters=cap, et_period=et)
    ids = [dec.ring_post(d_y.data_ptr() + 4 * N * lo, 32, rpk.data_ptr() + dec.KB * lo,
                         rit.data_ptr() + 4 * lo, rsy.data_ptr() + 4 * lo) for lo in (0, 32)]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    _check("%s ring cap %d et %d" % (name, cap, et), ref, rpk.cpu().numpy(), rit.cpu().numpy(),
           rsy.cpu().numpy())
    dec.close()
