"""GPU: ldpc_random_bits, ldpc_bpsk_awgn and ldpc_count_bit_errors against
tests/channel_ref.py (pinned on the CPU by tests/test_channel_ref_host.py).

The bits, the BPSK map, the composition out = fl(fl(2b - 1) + fl(sigma * n))
and the counts are held to the bit.  The normal deviates themselves come from
the device library's logf, sqrtf and sincospif and are held to the float64
restatement within ULP_LIMIT float32 ulps.

channel_ref.ULP_LIMIT is the largest error measured on an MI355X over the
three draws of test_awgn_deviates, 3.151 ulp (profiles/round25/channel.txt, by
sample position), plus 2 ulp for a revision of the device library.

Every device buffer is 64 elements longer than the call is told and holds a
sentinel there, which must survive the call."""
import math

import numpy as np
import pytest

import channel_ref as cr

pytestmark = pytest.mark.gpu

ULP_LIMIT = cr.ULP_LIMIT
GUARD = 64
NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4097, (1 << 20) + 3]
# pairs that differ in the high word only: (0, 2^32), (2^32 - 1, 2^64 - 1);
# in the low word only: (0, 1), (0, 2^32 - 1), (1, 2^32 - 1)
SEEDS = [0, 1, (1 << 32) - 1, 1 << 32, 0x0123456789ABCDEF, (1 << 64) - 1]
SENTINEL_U8 = 0xA5
SENTINEL_32 = 0x7FC0BEEF            # a quiet NaN as float, a large count as int32


class Buf:
    """n elements of `dtype` (uint8, int32 or float32) on the device with GUARD
    sentinel elements behind them."""

    def __init__(self, n, dtype, data=None):
        import torch
        self.n = int(n)
        if dtype == np.uint8:
            self.t = torch.full((self.n + GUARD,), SENTINEL_U8, dtype=torch.uint8, device="cuda:0")
        else:
            self.t = torch.full((self.n + GUARD,), SENTINEL_32, dtype=torch.int32, device="cuda:0")
        self.dtype = dtype
        if data is not None:
            src = np.ascontiguousarray(data, dtype).reshape(-1)
            assert src.size == self.n
            if self.n:
                v = src if dtype == np.uint8 else src.view(np.int32)
                self.t[:self.n] = torch.from_numpy(v.copy()).cuda(0)
        torch.cuda.synchronize()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """The first n elements; asserts that the sentinel survived."""
        import torch
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        want = SENTINEL_U8 if self.dtype == np.uint8 else SENTINEL_32
        assert (a[self.n:] == want).all(), "sentinel behind element %d overwritten" % self.n
        return a[:self.n].view(self.dtype).copy()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        want = SENTINEL_U8 if self.dtype == np.uint8 else SENTINEL_32
        return bool((self.t.cpu().numpy() == want).all())


# ---- random_bits ---------------------------------------------------------------------

def test_seed_set_has_the_pairs_it_needs():
    hi = [(a, b) for a in SEEDS for b in SEEDS if a < b and a & 0xFFFFFFFF == b & 0xFFFFFFFF]
    lo = [(a, b) for a in SEEDS for b in SEEDS if a < b and a >> 32 == b >> 32]
    assert len(hi) >= 2 and len(lo) >= 2


@pytest.mark.parametrize("seed", SEEDS)
def test_random_bits_bit_for_bit(seed):
    from ldpc_ece535a import _capi
    for n in NS:
        out = Buf(n, np.uint8)
        _capi.random_bits(out.ptr, n, seed)
        got = out.get()
        want = cr.random_bits(n, seed)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "n %d: %d bytes differ, first at %d (counter %d, word %d)" % (
            n, bad.size, bad[0], bad[0] >> 2, bad[0] & 3)


def test_random_bits_seeds_give_different_draws():
    """A dropped seed word would make two of the seeds draw the same bits."""
    draws = [cr.random_bits(4097, s) for s in SEEDS]
    for i in range(len(SEEDS)):
        for j in range(i):
            assert (draws[i] != draws[j]).sum() > 1500


def test_random_bits_n_zero_writes_nothing():
    from ldpc_ece535a import _capi
    out = Buf(0, np.uint8)
    _capi.random_bits(out.ptr, 0, 5)       # raises unless LDPC_OK
    assert out.untouched()
    _capi.random_bits(None, 0, 5)


# ---- bpsk_awgn -----------------------------------------------------------------------

def _all_bytes(n):
    """Every byte value, high bits set in most: the kernel may read bit 0 only."""
    return ((np.arange(n, dtype=np.int64) * 37 + 201) & 255).astype(np.uint8)


def test_awgn_sigma_zero_is_the_bpsk_map():
    from ldpc_ece535a import _capi
    assert set(_all_bytes(1023)) == set(range(256))
    for n in NS:
        b = _all_bytes(n)
        bits, out = Buf(n, np.uint8, b), Buf(n, np.float32)
        _capi.bpsk_awgn(bits.ptr, n, 0.0, 77, out.ptr)
        got = out.get()
        want = 2.0 * (b & 1).astype(np.float32) - 1.0
        assert got.tobytes() == want.tobytes(), "n %d" % n
        assert (bits.get() == b).all()


def test_awgn_n_zero_writes_nothing():
    from ldpc_ece535a import _capi
    bits, out = Buf(0, np.uint8), Buf(0, np.float32)
    _capi.bpsk_awgn(bits.ptr, 0, 1.0, 5, out.ptr)
    assert out.untouched() and bits.untouched()


N_BIG = (1 << 20) + 3
AWGN_SEEDS = [9, (3 << 32) | 7, (1 << 64) - 1]
_runs = {}


def _run(bits, n, sigma, seed):
    from ldpc_ece535a import _capi
    b, out = Buf(n, np.uint8, bits), Buf(n, np.float32)
    _capi.bpsk_awgn(b.ptr, n, sigma, seed, out.ptr)
    return out.get()


def scaled_run(seed):
    """One sigma = 2^40 run of N_BIG samples per seed, with its reference, shared
    by the tests below: dict(bits, out, n_ref)."""
    if seed not in _runs:
        # the bits of ldpc_random_bits at the same seed: a noise draw that landed
        # on their stream would show as deviates that follow the data
        bits = cr.random_bits(N_BIG, seed)
        _runs[seed] = dict(bits=bits, out=_run(bits, N_BIG, cr.SIGMA_BIG, seed),
                           n_ref=cr.normals_f64(N_BIG, seed))
    return _runs[seed]


@pytest.mark.parametrize("seed", AWGN_SEEDS)
def test_awgn_deviates(seed):
    """sigma = 2^40: the kernel's deviates, recovered to the bit wherever
    |n_ref| >= 2^-14, within ULP_LIMIT ulps of the float64 restatement; the few
    other samples within 2^-34 + 2^-40 absolutely (channel_ref.check_scaled_run)."""
    r = scaled_run(seed)
    n_ref = r["n_ref"]
    # the reference's own share of samples below 2^-14: 2 * 2^-14 * phi(0) = 4.87e-5
    # of the draw, 51 samples of 2^20, within five standard deviations (sqrt(51))
    small = int((np.abs(n_ref) < cr.SMALL).sum())
    want = 2 * cr.SMALL / math.sqrt(2 * math.pi) * N_BIG
    assert abs(small - want) <= 5 * math.sqrt(want), small
    loose = cr.check_scaled_run(r["out"], n_ref, float("inf"))
    print("seed %#x: max ulp by position (a cos, a sin, b cos, b sin) %s; share below 2^-14 %.3e"
          % (seed, ["%.3f" % v for v in loose["max_ulp_by_position"]], loose["small_share"]))
    res = cr.check_scaled_run(r["out"], n_ref, ULP_LIMIT)
    assert np.abs(res["n_dev"]).max() <= cr.BOUND
    assert res["small_share"] == small / N_BIG


@pytest.mark.parametrize("seed", AWGN_SEEDS[:2])
def test_awgn_composition_bit_for_bit(seed):
    """out == fl(fl(2b - 1) + fl(sigma * n_dev)) with the deviates of another
    run: the BPSK map, the pairing of bit and deviate, run-to-run determinism
    and the build without contraction (a fused multiply-add rounds once)."""
    from ldpc_ece535a import ber
    r = scaled_run(seed)
    ok = np.abs(r["n_ref"]) >= cr.SMALL
    n_dev = r["out"] * np.float32(2.0 ** -40)
    for sigma in (np.float32(0.7), np.float32(ber.sigma_of(2.0)), np.float32(1.0)):
        got = _run(r["bits"], N_BIG, float(sigma), seed)
        want = cr.compose(r["bits"], sigma, n_dev)
        bad = np.nonzero((got.view(np.int32) != want.view(np.int32)) & ok)[0]
        assert bad.size == 0, "sigma %r: %d samples differ, first %d: %r, want %r" % (
            float(sigma), bad.size, bad[0], float(got[bad[0]]), float(want[bad[0]]))
        # the samples not recovered: within the deviate's own tolerance
        rest = np.abs(got[~ok].astype(np.float64) - cr.bpsk(r["bits"][~ok]) -
                      float(sigma) * r["n_ref"][~ok])
        assert (rest <= 2.0 ** -23).all()


def test_awgn_tails_of_every_length():
    """n % 4 != 0 and short draws: a prefix of the long draw, to the bit."""
    seed = AWGN_SEEDS[0]
    r = scaled_run(seed)
    for n in NS[:-1]:
        got = _run(r["bits"][:n], n, cr.SIGMA_BIG, seed)
        assert got.tobytes() == r["out"][:n].tobytes(), "n %d" % n


def test_awgn_extreme_draws():
    """Draws found on the CPU with the restatement (tests/test_channel_ref_host.py,
    EXTREMES): (seed, counter) whose u1 rounds to 1.0 -- noise exactly 0 at any
    sigma --, whose u1 is 45 * 2^-32 -- radius 6.06 --, whose u2 rounds to 1.0 --
    sin(2 pi) = 0 exactly, cos = 1."""
    seed, ctr = 235, 16976                       # x = 0xfffffff2: samples 67904, 67905
    n = 4 * ctr + 4
    bits = cr.random_bits(n, 1)
    for sigma in (0.7, 1.0, cr.SIGMA_BIG):
        got = _run(bits, n, sigma, seed)[4 * ctr:]
        assert (got[:2] == cr.bpsk(bits[4 * ctr:4 * ctr + 2])).all(), (sigma, got)
        assert (got[2:] != cr.bpsk(bits[4 * ctr + 2:])).all()
    print("u1 -> 1 (seed 235, samples 67904..67907, sigma 2^40): %r" % (list(got),))

    seed, ctr = 118, 212107                      # x = 0x2c: u1 = 45 * 2^-32
    n = 4 * ctr + 4
    bits = cr.random_bits(n, 1)
    n_ref = cr.normals_f64(n, seed)
    out = _run(bits, n, cr.SIGMA_BIG, seed)
    n_dev = out[4 * ctr:] * np.float32(2.0 ** -40)
    print("small u1 (seed 118, samples 848428..848431): %r" % (list(n_dev),))
    assert (cr.ulp_error(n_dev, n_ref[4 * ctr:]) <= ULP_LIMIT).all()
    radius = math.hypot(float(n_dev[0]), float(n_dev[1]))
    assert abs(radius - math.sqrt(-2 * math.log(45 * 2.0 ** -32))) < 1e-5 and radius > 6.06
    assert np.abs(n_dev).max() <= cr.BOUND

    seed, ctr = 143, 14990                       # y = 0xffffffd3: u2 = 1.0 in pair a
    n = 4 * ctr + 4
    bits = cr.random_bits(n, 1)
    n_ref = cr.normals_f64(n, seed)
    assert n_ref[4 * ctr + 1] == 0
    for sigma in (0.7, cr.SIGMA_BIG):
        got = _run(bits, n, sigma, seed)
        assert got[4 * ctr + 1] == cr.bpsk(bits[4 * ctr + 1])        # r * sin(2 pi) == 0
    n_dev = got[4 * ctr:] * np.float32(2.0 ** -40)
    print("u2 -> 1 (seed 143, samples 59960..59963): %r" % (list(n_dev),))
    assert cr.ulp_error(n_dev[0], n_ref[4 * ctr]) <= ULP_LIMIT       # r * cos(2 pi) == r


# ---- count_bit_errors ----------------------------------------------------------------

PER_FRAME = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099]


def _count(a, b, per_frame, B):
    from ldpc_ece535a import _capi
    da, db = Buf(B * per_frame, np.uint8, a), Buf(B * per_frame, np.uint8, b)
    cnt = Buf(B, np.int32)
    _capi.count_bit_errors(da.ptr, db.ptr, per_frame, B, cnt.ptr)
    got = cnt.get()
    assert (da.get() == a.reshape(-1)).all() and (db.get() == b.reshape(-1)).all()
    return got


@pytest.mark.parametrize("B", [1, 2, 77])
def test_count_bit_errors(B):
    rng = np.random.default_rng(25)
    for pf in PER_FRAME:
        shape = (B, pf)
        a = rng.integers(0, 2, shape, dtype=np.uint8)
        flips = (rng.random(shape) < 0.03).astype(np.uint8)
        what = "per_frame %d" % pf
        # random 0/1 bytes, 3 % flipped
        assert (_count(a, a ^ flips, pf, B) == flips.sum(axis=1)).all(), what
        # all equal, all different
        assert (_count(a, a.copy(), pf, B) == 0).all(), what
        assert (_count(a, a ^ 1, pf, B) == pf).all(), what
        # only bit 0 counts: high bits that differ, and high bits that agree
        hi = (rng.integers(0, 128, shape, dtype=np.uint8) << 1).astype(np.uint8)
        hi2 = (rng.integers(1, 128, shape, dtype=np.uint8) << 1).astype(np.uint8)
        assert (_count(a | hi, a | (hi ^ hi2), pf, B) == 0).all(), what
        assert (_count(a | hi, (a ^ flips) | hi, pf, B) == flips.sum(axis=1)).all(), what
        assert (_count(a | hi, (a ^ flips) | (hi ^ hi2), pf, B) == flips.sum(axis=1)).all(), what
        # a frame's count takes nothing from its neighbours: all different next to all equal
        for first in (0, 1):
            odd = ((np.arange(B) + first) & 1).astype(np.uint8)[:, None]
            assert (_count(a, a ^ odd, pf, B) == odd[:, 0].astype(np.int64) * pf).all(), what


def test_count_bit_errors_no_frames():
    from ldpc_ece535a import _capi
    a, cnt = Buf(16, np.uint8), Buf(0, np.int32)
    _capi.count_bit_errors(a.ptr, a.ptr, 16, 0, cnt.ptr)
    assert cnt.untouched()
