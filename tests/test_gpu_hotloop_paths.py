"""The exact sum-product loop's reformulated paths (csrc/ldpc_exact.hpp,
ldpc_device.hpp log_ratio_n_packed), each forced to run, against the oracle.

One batch of B = 192 frames of the default H (three full waves of lanes'
worth), decoded through `decode` (posteriors too), `decode_device` and one
ring session, at iteration caps 1, 5, 50 and et_period 1, 5.  The frames, by
the path each family forces:

  * 64 seeded frames at 2 dB -- the headline's mix: some near-1 ratios per
    iteration (one packed pass), the q == 1 cells of the padding edges and
    degree-1 columns (their +0 slot), +0.0 bit messages (tanh's general path).
  * |y| = 0.05 everywhere -- every bit message is small, every real check
    product T is tiny but not 0, so all 168 ratios (1 + T) / (1 - T) are near
    1 and none equals 1: more than 128 packed operands, three dense passes per
    iteration, and positions from all three slots' masks (the scalar AND of
    the near-1 and not-unit ballots).
  * |y| = 2^-60 -- bit messages below 2^-54: tanh's special branch in every
    wave (the mask formed from two ballots, and its scalar copy for the test
    after the divisions); T underflows far below 2^-54, so q = 1 on every
    lane: no packed operand at all, every lane reads the +0 slot.
  * |y| = 30 -- |m| >= 13.5: expm1's k >= 20 formula (mid_possible, taken
    only through tanh's special flag) and k > 0 on every lane (the numerator
    select and the -1 addend read by k).
  * |y| = 45 -- |m| >= 38.2: tanh = +-1 exactly, T = +-1, the division batch
    with raised divisors and infinite check messages (ratio_fix_n).
  * mixed -- those magnitudes and +-0.0 within one frame: lanes of one wave on
    different paths in the same instruction (k > 0 next to k <= 0, special next
    to general, packed next to unit next to main-path logs).
  * an infinity and a NaN sample -- the non-FIN loop (selects on missing
    edges) running the same functions.

Half of each constant-magnitude family carries the signs of noisy codewords
(frames that converge), half random signs (frames that run to the cap).  A
second test runs a code with two column words (hData2, N = 100: NW = 2, the
edge-form loop and its tanh_half_n<S>) at B = 64 on random samples.

Everything compared is exact: packed bytes, iteration counts, syndrome
weights, and the posteriors' bit patterns (NaN == NaN)."""
import os

import numpy as np
import pytest

import ldpc_ece535a as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 192
_cache = {}


def _noisy(Hr, n, db, rng):
    data = rng.integers(0, 2, size=(n, Hr.shape[1] - Hr.shape[0]), dtype=np.uint8)
    x = 2.0 * L.encode(Hr, data) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


def _frames(Hr):
    """the batch, built once and read only"""
    if "y" not in _cache:
        rng = np.random.Generator(np.random.PCG64(7007))
        N = Hr.shape[1]
        parts = [_noisy(Hr, 64, 2.0, rng)]

        def signs(n):
            s = np.sign(_noisy(Hr, n, 2.0, rng)).astype(np.float32)
            s[s == 0] = 1.0
            s[n // 2:] = rng.choice(np.float32([-1.0, 1.0]), size=(n - n // 2, N))
            return s

        mags = np.float32([0.05, 2.0 ** -60, 30.0, 45.0])
        for a in mags:
            parts.append(signs(24) * a)
        mix = signs(24) * rng.choice(np.concatenate([mags, np.float32([0.0, 1.0])]), size=(24, N))
        mix[:, 3] = -0.0
        mix[::2, 40] = 0.0
        parts.append(mix.astype(np.float32))
        nf = np.concatenate([_noisy(Hr, 4, 2.0, rng), mix[:4]]).astype(np.float32)
        nf[:, 7] = np.inf
        nf[:, 21] = np.nan
        nf[1, 50] = -np.inf
        nf[2, 7] = 1.0  # a NaN alone
        nf[3, 21] = 1.0  # an infinity alone
        parts.append(nf)
        y = np.ascontiguousarray(np.concatenate(parts), np.float32)
        assert y.shape == (B, N)
        y.setflags(write=False)
        _cache["y"] = y
    return _cache["y"]


def _oracle(key, method, Hr, y, iters, et):
    from oracle import oracle as orc
    if key not in _cache:
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
        _cache[key] = orc.decode_batch(method, Hr, y, iters, nthreads=threads, et_period=et,
                                       want_post=True)
    return _cache[key]


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _check(name, ref, packed, iters, synd, llr=None):
    bad = np.flatnonzero((packed != ref["packed"]).any(axis=1))
    assert bad.size == 0, (name, "packed bytes differ on frames", bad[:8])
    np.testing.assert_array_equal(iters, ref["iters"], err_msg=name)
    np.testing.assert_array_equal(synd, ref["synd"], err_msg=name)
    if llr is not None:
        same = _same_bits(llr, ref["post"])
        assert same.all(), (name, "posteriors differ at", np.argwhere(~same)[:5])


def _three_ways(dec, y, ref, iters, et):
    n, N = y.shape
    out = dec.decode(y, method=1, max_iters=iters, et_period=et, want_llr=True)
    _check("decode", ref, out["packed"], out["iters"], out["synd"], out["llr"])

    d_y = torch.from_numpy(np.array(y)).cuda()
    pk = torch.zeros((n, dec.KB), dtype=torch.uint8, device="cuda")
    it = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sy = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ll = torch.zeros((n, N), dtype=torch.float32, device="cuda")
    dec.decode_device(d_y.data_ptr(), n, pk.data_ptr(), method=1, max_iters=iters, et_period=et,
                      d_iters=it.data_ptr(), d_synd=sy.data_ptr(), d_llr=ll.data_ptr())
    dec.synchronize()
    _check("decode_device", ref, pk.cpu().numpy(), it.cpu().numpy(), sy.cpu().numpy(),
           ll.cpu().numpy())

    rpk, rit, rsy = torch.zeros_like(pk), torch.full_like(it, -1), torch.full_like(sy, -1)
    torch.cuda.synchronize()
    dec.ring_begin(method=1, max_iters=iters, et_period=et)
    half = n // 2
    ids = [dec.ring_post(d_y.data_ptr() + 4 * N * lo, hi - lo, rpk.data_ptr() + dec.KB * lo,
                         rit.data_ptr() + 4 * lo, rsy.data_ptr() + 4 * lo)
           for lo, hi in ((0, half), (half, n))]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    _check("ring", ref, rpk.cpu().numpy(), rit.cpu().numpy(), rsy.cpu().numpy())


@pytest.mark.parametrize("et", [1, 5])
@pytest.mark.parametrize("iters", [1, 5, 50])
def test_hot_loop_paths_vs_oracle(iters, et):
    dec = L.Decoder()
    y = _frames(dec.H)
    ref = _oracle(("default", iters, et), 1, dec.H, y, iters, et)
    _three_ways(dec, y, ref, iters, et)
    dec.close()


def test_two_column_words_vs_oracle():
    """hData2 (N = 100): NW = 2, the edge-form sum-product loop."""
    from ldpc_ece535a import codes
    from oracle import oracle as orc
    M, N, rp, ci = codes.read_alist(os.path.join(os.path.dirname(__file__), "golden",
                                                 "hData2.alist"))
    H = np.zeros((M, N), np.uint8)
    for j in range(M):
        H[j, ci[rp[j]:rp[j + 1]]] = 1
    dec = L.Decoder(H)
    Hr = orc.reorder_h(H)[0]
    assert (dec.H == Hr).all() and dec.N > 64
    rng = np.random.Generator(np.random.PCG64(7008))
    y = _noisy(Hr, 64, 2.0, rng)
    y.setflags(write=False)
    for iters, et in ((50, 1), (5, 5)):
        ref = _oracle(("hData2", iters, et), 1, Hr, y, iters, et)
        _three_ways(dec, y, ref, iters, et)
    dec.close()
