"""The column-centric sum-product loop decides a frame's exit before the tanh
pass (csrc/ldpc_frame.hpp, the kCols loop): a last iteration, at the cap or on
a zero syndrome, computes no operands for a next one.  Every result has to
stay what it was: iterations, syndrome weight, hard bits, posteriors, packed
bytes.

One batch of B = 192 frames of the default H, interleaved so that consecutive
frames end differently (frame 3k: converging, 3k + 1: runs to the cap, 3k + 2:
holds a non-finite sample):

  * converging: 16 noiseless codewords (exit at iteration 1) and 48 frames at
    2 dB whose oracle decode at cap 50 ends with syndrome 0 after u iterations,
    2 <= u <= 12, taken in order from a seeded pool;
  * runs to the cap: 64 frames of that pool with a non-zero syndrome after 50;
  * non-finite: 64 frames at 2 dB with an infinity (even k) or a NaN (odd k)
    at a position that moves with k -- the non-FIN instantiation.

Decoded through `decode` (posteriors as bit patterns, NaN == NaN),
`decode_device` and a ring session:

  * at every cap 1 .. 13 and at 50: for a frame converging at u these hold
    u - 1 (the cap ends it one iteration early), u (both exit conditions at
    once) and u + 1; cap 1 runs no tanh pass after the initial one;
  * et_period 5 at cap 50 (frames converging at 2 run to 5), 7 at cap 50 (the
    period does not divide the cap), 64 at cap 10 (no early exit at all);
  * three batches of 4 100 frames, the 192 tiled, in one ring session at cap
    6: a persistent wave decodes frames that end by the cap, by convergence
    and in the non-finite loop one after another.

Precisions 0 and 2 are compared with the oracle exactly.  Precisions 1 and 3
have no exact oracle: their iteration count at cap c must be min(c, the count
at cap 50), their bytes at a cap at or above a frame's own count must be the
cap-50 bytes, the three entry points must agree, and packed bytes, iterations
and syndromes at caps 1, 5 and 50 must equal what the commit before this
change produced (tests/golden/exit_order_prec13.npz, recorded on an MI355X)."""
import hashlib
import os

import numpy as np
import pytest

import ldpc_ece535a as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 192
CAPS = list(range(1, 14)) + [50]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "exit_order_prec13.npz")
_cache = {}


def _noisy(Hr, n, db, rng):
    data = rng.integers(0, 2, size=(n, Hr.shape[1] - Hr.shape[0]), dtype=np.uint8)
    x = 2.0 * L.encode(Hr, data) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _frames(Hr):
    """(y, u): the batch, built once and read only, and the oracle's iteration
    count at cap 50 of each frame (0 where the frame does not converge)."""
    if "y" not in _cache:
        from oracle import oracle as orc
        rng = np.random.Generator(np.random.PCG64(9011))
        N = Hr.shape[1]
        pool = _noisy(Hr, 384, 2.0, rng)
        ref = orc.decode_batch(1, Hr, pool, 50, nthreads=_threads())
        conv = np.flatnonzero((ref["synd"] == 0) & (ref["iters"] >= 2) & (ref["iters"] <= 12))
        capped = np.flatnonzero((ref["synd"] != 0) & (ref["iters"] == 50))
        assert conv.size >= 48 and capped.size >= 64, (conv.size, capped.size)
        clean = np.sign(_noisy(Hr, 16, 40.0, rng)).astype(np.float32)
        g0 = np.concatenate([clean, pool[conv[:48]]])
        # noiseless codewords among the others, not in a block of their own
        g0 = g0[np.argsort(np.arange(64) % 4, kind="stable")]
        g1 = pool[capped[:64]]
        g2 = _noisy(Hr, 64, 2.0, rng)
        for k in range(64):
            g2[k, (7 * k + 3) % N] = (np.inf if k % 4 == 0 else -np.inf) if k % 2 == 0 else np.nan
        y = np.empty((B, N), np.float32)
        y[0::3], y[1::3], y[2::3] = g0, g1, g2
        y.setflags(write=False)
        r50 = _oracle(50, 1, Hr, y)
        u = np.where(r50["synd"] == 0, r50["iters"], 0)
        _cache["y"] = (y, u)
    return _cache["y"]


def _oracle(cap, et, Hr, y):
    from oracle import oracle as orc
    if (cap, et) not in _cache:
        _cache[(cap, et)] = orc.decode_batch(1, Hr, y, cap, nthreads=_threads(), et_period=et,
                                             want_post=True)
    return _cache[(cap, et)]


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


def _three_ways(dec, y, cap, et, prec):
    """the batch through decode, decode_device and a ring session of two
    posts; returns the three results (decode's first)"""
    n, N = y.shape
    out = dec.decode(y, method=1, max_iters=cap, et_period=et, precision=prec, want_llr=True)
    res = [("decode", dict(packed=out["packed"], iters=out["iters"], synd=out["synd"],
                           post=out["llr"]))]

    d_y = torch.from_numpy(np.array(y)).cuda()
    pk = torch.zeros((n, dec.KB), dtype=torch.uint8, device="cuda")
    it = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sy = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ll = torch.zeros((n, N), dtype=torch.float32, device="cuda")
    dec.decode_device(d_y.data_ptr(), n, pk.data_ptr(), method=1, max_iters=cap, et_period=et,
                      precision=prec, d_iters=it.data_ptr(), d_synd=sy.data_ptr(),
                      d_llr=ll.data_ptr())
    dec.synchronize()
    res.append(("decode_device", dict(packed=pk.cpu().numpy(), iters=it.cpu().numpy(),
                                      synd=sy.cpu().numpy(), post=ll.cpu().numpy())))

    rpk, rit, rsy = torch.zeros_like(pk), torch.full_like(it, -1), torch.full_like(sy, -1)
    torch.cuda.synchronize()
    dec.ring_begin(method=1, max_iters=cap, et_period=et, precision=prec)
    half = n // 2
    ids = [dec.ring_post(d_y.data_ptr() + 4 * N * lo, hi - lo, rpk.data_ptr() + dec.KB * lo,
                         rit.data_ptr() + 4 * lo, rsy.data_ptr() + 4 * lo)
           for lo, hi in ((0, half), (half, n))]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    res.append(("ring", dict(packed=rpk.cpu().numpy(), iters=rit.cpu().numpy(),
                             synd=rsy.cpu().numpy())))
    return res


def _exact(dec, y, cap, et, prec):
    ref = _oracle(cap, et, dec.H, y)
    for name, r in _three_ways(dec, y, cap, et, prec):
        _check("%s cap %d et %d prec %d" % (name, cap, et, prec), ref, r["packed"], r["iters"],
               r["synd"], r.get("post"))
    return ref


def test_batch_holds_the_cases():
    """the frames this file relies on exist (CPU oracle only)"""
    dec = L.Decoder()
    y, u = _frames(dec.H)
    r50 = _oracle(50, 1, dec.H, y)
    assert ((u >= 2) & (u <= 12)).sum() >= 16  # cap and convergence can meet
    assert (u == 1).sum() >= 16  # noiseless: exit at iteration 1
    assert (u == 2).sum() >= 1  # et_period 5: these run to 5
    assert (r50["iters"][1::3] == 50).all() and (r50["synd"][1::3] != 0).all()
    assert (~np.isfinite(y[2::3])).any(axis=1).all() and np.isfinite(y[0::3]).all()
    r5 = _oracle(50, 5, dec.H, y)
    assert (r5["iters"][(u >= 1) & (u <= 5)] == 5).all()
    dec.close()


@pytest.mark.parametrize("prec", [L.PREC_F64, L.PREC_F64_LIBM])
@pytest.mark.parametrize("cap", CAPS)
def test_caps_vs_oracle(cap, prec):
    """caps u - 1, u, u + 1 of every converging frame (u = 2 .. 12), cap 1,
    cap 50; the non-finite frames at every cap (1 and 5 among them)"""
    dec = L.Decoder()
    y, u = _frames(dec.H)
    ref = _exact(dec, y, cap, 1, prec)
    # what the oracle itself says at this cap: the cap ends a frame that would
    # converge later, and a frame converging at the cap stops there with both
    # exit conditions true
    late = u > cap
    assert (ref["iters"][late] == cap).all()
    meet = u == cap
    assert (ref["iters"][meet] == cap).all() and (ref["synd"][meet] == 0).all()
    dec.close()


@pytest.mark.parametrize("prec", [L.PREC_F64, L.PREC_F64_LIBM])
@pytest.mark.parametrize("et,cap", [(5, 50), (7, 50), (64, 10)])
def test_et_period_vs_oracle(et, cap, prec):
    dec = L.Decoder()
    y, u = _frames(dec.H)
    ref = _exact(dec, y, cap, et, prec)
    if et == 64:
        assert (ref["iters"] == cap).all()  # never a multiple of the period
    else:
        assert ((ref["iters"] % et == 0) | (ref["iters"] == cap)).all()
    dec.close()


@pytest.mark.parametrize("prec", [L.PREC_F64, L.PREC_F64_LIBM])
def test_ring_wave_decodes_frames_in_a_row(prec):
    """three batches of 4 100 frames in one session at cap 6: whatever a wave
    keeps from one frame to the next serves frames ending by the cap, by
    convergence and in the non-finite loop alike"""
    dec = L.Decoder()
    y, _ = _frames(dec.H)
    ref = _oracle(6, 1, dec.H, y)
    n, N = 4100, y.shape[1]
    idx = np.arange(n) % B
    d_y = torch.from_numpy(np.ascontiguousarray(y[idx])).cuda()
    outs = [(torch.zeros((n, dec.KB), dtype=torch.uint8, device="cuda"),
             torch.full((n,), -1, dtype=torch.int32, device="cuda"),
             torch.full((n,), -1, dtype=torch.int32, device="cuda")) for _ in range(3)]
    torch.cuda.synchronize()
    dec.ring_begin(method=1, max_iters=6, precision=prec)
    ids = [dec.ring_post(d_y.data_ptr(), n, pk.data_ptr(), it.data_ptr(), sy.data_ptr())
           for pk, it, sy in outs]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    tiled = dict(packed=ref["packed"][idx], iters=ref["iters"][idx], synd=ref["synd"][idx])
    for k, (pk, it, sy) in enumerate(outs):
        _check("ring batch %d prec %d" % (k, prec), tiled, pk.cpu().numpy(), it.cpu().numpy(),
               sy.cpu().numpy())
    dec.close()


def frames_digest(y):
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


@pytest.mark.parametrize("prec", [L.PREC_F32, L.PREC_F64_FAST])
def test_inexact_precisions(prec):
    dec = L.Decoder()
    y, _ = _frames(dec.H)
    gold = np.load(GOLDEN)
    assert str(gold["frames_sha256"]) == frames_digest(y), "the fixture was recorded on other frames"
    got = {}
    for cap in (1, 2, 5, 50):
        res = _three_ways(dec, y, cap, 1, prec)
        first = res[0][1]
        for name, r in res[1:]:  # the entry points agree
            _check("%s vs decode, cap %d prec %d" % (name, cap, prec), first, r["packed"],
                   r["iters"], r["synd"], r.get("post"))
        got[cap] = first
    full = got[50]
    for cap in (1, 2, 5):
        np.testing.assert_array_equal(got[cap]["iters"], np.minimum(cap, full["iters"]))
    for cap in (1, 2, 5, 50):
        done = full["iters"] <= cap  # the cap does not cut these short
        assert (got[cap]["packed"][done] == full["packed"][done]).all(), cap
        np.testing.assert_array_equal(got[cap]["synd"][done], full["synd"][done])
    for cap in (1, 5, 50):  # unchanged from the commit before
        for f in ("packed", "iters", "synd"):
            np.testing.assert_array_equal(got[cap][f], gold["p%d_c%d_%s" % (prec, cap, f)],
                                          err_msg="cap %d %s" % (cap, f))
    dec.close()
