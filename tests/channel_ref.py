"""The channel routines of csrc/ldpc_aux.hip restated in numpy.

`k_random_bits` and `k_bpsk_awgn` draw from Philox4x32-10 (Salmon et al.,
"Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known
answers pin `philox4x32_10` in tests/test_channel_ref_host.py).  Thread t of
either kernel owns samples 4t .. 4t+3 and makes one draw for them:

    counter = (ctr & 0xFFFFFFFF, ctr >> 32, stream, 0x2545F491),  ctr = i >> 2
    key     = (seed & 0xFFFFFFFF, seed >> 32)
    stream  = 1 for random_bits, 2 for bpsk_awgn

random_bits: byte i = bit 31 of word i & 3.

bpsk_awgn: words (x, y) make Box-Muller pair a, words (z, w) pair b, in float:

    u1 = min(fl(fl(fl(x) + 1) * 2^-32), 1)        in (0, 1]
    u2 = fl(y) * 2^-32                            in [0, 1]     (pair b: z, w)
    r  = sqrtf(-2 logf(u1));  (s, c) = sincospif(2 u2)
    n[4c + 0] = ra * ca,  n[4c + 1] = ra * sa,  n[4c + 2] = rb * cb,  n[4c + 3] = rb * sb
    out[i] = fl(fl(2 (bits[i] & 1) - 1) + fl(sigma * n[i]))    (no contraction)

Everything up to u1, u2 is integer or exact float arithmetic and is restated
to the bit.  `normals_f64` evaluates r, s, c in float64 from those float32
uniforms: the yardstick the kernel's deviates are measured against in float32
ulps (`ulp_error`, `check_scaled_run`).  u1 >= 2^-32 bounds every deviate by
sqrt(2 * 32 * ln 2) = 6.6604.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
COUNTER_W = 0x2545F491
STREAM_BITS, STREAM_NOISE = 1, 2
MASK = np.uint64(0xFFFFFFFF)
TWO_M32 = np.float32(2.0 ** -32)
BOUND = math.sqrt(2 * 32 * math.log(2.0))     # the largest radius: u1 = 2^-32
SMALL = 2.0 ** -14                             # below it the +-1 shows in a sigma = 2^40 run
SIGMA_BIG = 2.0 ** 40
# The limit the kernel's deviates are held to, in float32 ulps of the float64 value: the
# largest error measured on an MI355X over three draws of 2^20 + 3 samples, 3.151 ulp
# (profiles/round25/channel.txt, by sample position), plus 2 ulp for a revision of the
# device library.  logf, sqrtf and sincospif at no more than 1 ulp each and one rounded
# product predict 3 to 4.
ULP_LIMIT = 3.151 + 2.0


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit words held in uint64;
    returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(v, np.uint64)) & MASK
                              for v in (c0, c1, c2, c3, k0, k1))
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> sh) ^ c1 ^ k0, p1 & MASK, (p0 >> sh) ^ c3 ^ k1, p0 & MASK)
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def draw(n4, stream, seed, ctr=None):
    """(n4, 4) uint64 words: row c is the draw of counter ctr[c] (default c)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.arange(n4, dtype=np.uint64) if ctr is None else np.asarray(ctr, np.uint64)
    w = philox4x32_10(ctr & MASK, ctr >> np.uint64(32), stream, COUNTER_W,
                      seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1)


def _n4(n):
    return (int(n) + 3) // 4


def random_bits(n, seed):
    """ldpc_random_bits: n bytes, 0 or 1."""
    w = draw(_n4(n), STREAM_BITS, seed)
    return (w >> np.uint64(31)).astype(np.uint8).reshape(-1)[:n]


def uniforms_of(words):
    """(u1, u2), each (n4, 2) float32: column 0 is pair a (x, y), column 1 pair b (z, w)."""
    f = words.astype(np.uint32).astype(np.float32)     # nearest-even, as v_cvt_f32_u32
    u1 = np.minimum((f[:, 0::2] + np.float32(1.0)) * TWO_M32, np.float32(1.0))
    u2 = f[:, 1::2] * TWO_M32
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def uniforms(n, seed):
    return uniforms_of(draw(_n4(n), STREAM_NOISE, seed))


def _sincospi(t):
    """sin(pi t), cos(pi t) of float64 t in [0, 2], t a float32 value: t is
    split exactly into q / 2 + f, |f| <= 1/4, so the results keep their
    relative accuracy next to the zeros."""
    q = np.rint(2.0 * t)
    f = t - 0.5 * q                                    # exact
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    q = q.astype(np.int64) & 3
    sin = np.choose(q, [s, c, -s, -c])
    cos = np.choose(q, [c, -s, -c, s])
    return sin, cos


def normals_of(words):
    """(4 * n4,) float64 deviates of the (n4, 4) words, in the kernel's sample order."""
    u1, u2 = uniforms_of(words)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    s, c = _sincospi((np.float32(2.0) * u2).astype(np.float64))
    out = np.empty((words.shape[0], 4), np.float64)
    out[:, 0::2] = r * c
    out[:, 1::2] = r * s
    return out.reshape(-1)


def normals_f64(n, seed):
    return normals_of(draw(_n4(n), STREAM_NOISE, seed))[:n]


def ulp_error(got, ref):
    """|got - ref| in units of the float32 spacing at |ref| (float64 ref)."""
    got = np.asarray(got, np.float32).astype(np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def bpsk(bits):
    return np.float32(2.0) * (np.asarray(bits, np.uint8) & 1).astype(np.float32) - np.float32(1.0)


def check_scaled_run(out, n_ref, ulp_limit):
    """The comparison of a sigma = 2^40 run with the float64 deviates.

    2^40 * n is exact.  Where |n_ref| >= 2^-14 the product is at least 2^26,
    half a float32 ulp there is at least 4 and the added +-1 vanishes, so
    out * 2^-40 is the kernel's deviate to the bit: it must lie within
    ulp_limit float32 ulps of n_ref.  The other samples, at most 1e-3 of the
    draw, must satisfy |out * 2^-40 - n_ref| <= 2^-34 + 2^-40.  Returns
    dict(n_dev, big, ulps, max_ulp_by_position, small_share); raises
    AssertionError with the first offending sample."""
    out = np.asarray(out, np.float32)
    n_ref = np.asarray(n_ref, np.float64)
    assert out.shape == n_ref.shape and out.ndim == 1
    assert np.isfinite(out).all()
    n_dev = out * np.float32(2.0 ** -40)               # exact: no deviate is subnormal here
    big = np.abs(n_ref) >= SMALL
    ulps = np.where(big, ulp_error(n_dev, n_ref), 0.0)
    by_pos = [float(ulps[k::4].max()) if ulps[k::4].size else 0.0 for k in range(4)]
    share = float((~big).sum()) / max(out.size, 1)
    assert share <= 1e-3, "share of samples below 2^-14: %g" % share
    bad = np.nonzero(ulps > ulp_limit)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%d samples beyond %g ulp; first: sample %d (counter %d, position %d) "
                             "device %r reference %r (%.2f ulp)" %
                             (bad.size, ulp_limit, i, i >> 2, i & 3, float(n_dev[i]),
                              float(n_ref[i]), ulps[i]))
    rest = np.abs(out[~big].astype(np.float64) * 2.0 ** -40 - n_ref[~big])
    lim = 2.0 ** -34 + 2.0 ** -40
    if (rest > lim).any():
        i = int(np.nonzero(~big)[0][np.argmax(rest)])
        raise AssertionError("small sample %d: out * 2^-40 = %r, reference %r" %
                             (i, float(out[i]) * 2.0 ** -40, float(n_ref[i])))
    return dict(n_dev=n_dev, big=big, ulps=ulps, max_ulp_by_position=by_pos, small_share=share)


def compose(bits, sigma, n_dev):
    """fl(fl(2 b - 1) + fl(sigma * n_dev)) in float32: two roundings, no fused multiply-add."""
    prod = np.float32(sigma) * np.asarray(n_dev, np.float32)
    out = bpsk(bits) + prod
    assert prod.dtype == np.float32 and out.dtype == np.float32
    return out
