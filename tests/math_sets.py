"""Operand sets for the decoder's arithmetic, shared by the host tests
(tests/test_exact.py, tests/test_math.py, tests/test_math_sets_host.py) and
the device tests (tests/test_gpu_math.py): random sweeps, every double around
the boundaries of each branch of glibc's code, the special values and the hard
cases of division.

Every generator draws the same numbers whatever `cap` is (the cap cuts each
set after it has been drawn), so the host tests, which pass no cap, sweep what
they always did, and the device tests take the first `cap` operands of the
same sets."""
import numpy as np

GPU_CAP = 1 << 20   # operands per set on the device: a test takes a few seconds
WAVE = 64 * 3       # operands of one wave of ldpc_math_probe (three per lane)


def around(points, width=64):
    """every double within `width` ulp of each point, both signs"""
    pts = np.asarray(points, np.float64)
    b = pts.view(np.int64)[:, None] + np.arange(-width, width + 1)[None, :]
    v = b.view(np.float64).ravel()
    return np.concatenate([v, -v])


def triples(x, pad=0.5):
    x = np.asarray(x).ravel()
    n = (-x.size) % 3
    return np.concatenate([x, np.full(n, pad, x.dtype)]) if n else x


def _cut(sets, cap):
    return [s if cap is None else s[:cap] for s in sets]


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, 2.0 ** -55,
                     2.0 ** -54, 22.0, -22.0, 21.999, 1.0, -1.0, 0.34657359, 1.0397, 38.8,
                     44.0, 1e300, -1e300])


def inputs(seed, n=400_000):
    """tests/test_math.py's tanh operands"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n), rng.uniform(-30, 30, n), rng.normal(0, 8, n),
            rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-20, 0, n), SPECIALS]


# ---- tests/test_exact.py ---------------------------------------------------------------

def log_sets(cap=None):
    rng = np.random.default_rng(101)
    return _cut([rng.uniform(0, 3, 4_000_000), np.exp(rng.uniform(-45, 45, 4_000_000)),
                 1 + rng.uniform(-0.07, 0.07, 4_000_000),
                 1 + rng.uniform(-1, 1, 2_000_000) * 10.0 ** rng.uniform(-17, -1, 2_000_000),
                 10.0 ** rng.uniform(-307, 308, 2_000_000),
                 # both ends of the |x - 1| < 1/16 window and every table subinterval edge
                 around([1 - 2.0 ** -4, 1 + float.fromhex("0x1.09p-4"), 1.0], 4096),
                 around(np.arange(0x3FE6000000000000, 0x3FF6000000000000, 1 << 45,
                                  dtype=np.int64).view(np.float64), 16),
                 np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 2.0, 0.5, 5e-324, 1e-310,
                           -1.0])], cap)


def tanh_half_sets(cap=None):
    rng = np.random.default_rng(102)
    ln2 = np.log(2.0)
    # expm1's k classes switch at |u| = 0.5 ln2, 1.5 ln2 (high word) and
    # (k + 1/2) ln2; u = |m| (|m| >= 2) or -|m|; tanh's at |m| = 2, 44, 2^-54
    edges = [0.5 * ln2, 1.5 * ln2, 2.0, 44.0, 2.0 ** -54, 2.0 ** -53]
    edges += [(k + 0.5) * ln2 for k in range(2, 64)]
    edges += [float.fromhex("0x1.62e42p-2"), float.fromhex("0x1.0a2b2p0")]
    return _cut([rng.uniform(-4, 4, 6_000_000), rng.uniform(-60, 60, 6_000_000),
                 rng.normal(0, 12, 6_000_000),
                 rng.uniform(-1, 1, 3_000_000) * 10.0 ** rng.uniform(-30, 0, 3_000_000),
                 around(edges, 512),
                 # |m| with high word 0x3fd62e42 above 0.5 ln2, where glibc's expm1
                 # takes k = 0 by the high word and the rounding alone would not
                 # (ldpc_exact.hpp takes that select in a rare branch)
                 np.concatenate([v := rng.integers(0x3FD62E42FEFA39EF, 0x3FD62E4300000000, 200_000,
                                                    dtype=np.int64).view(np.float64), -v]),
                 np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, 1e300,
                           -1e300, 2.0, -2.0, 44.0, -44.0])], cap)


def expm1_sets(cap=None):
    rng = np.random.default_rng(103)
    out = []
    for u in (-rng.uniform(0, 2, 3_000_000), rng.uniform(2, 44, 3_000_000),
              -10.0 ** rng.uniform(-16, 0.3, 3_000_000)):
        out.append(u[((u < 0) & (u > -2) & (u <= -2.0 ** -54)) | ((u >= 2) & (u < 44))])
    return _cut(out, cap)


def log_ratio_sets(cap=None):
    """T in [-1, 1] or NaN: what a product of tanh values can be"""
    rng = np.random.default_rng(104)
    t = np.tanh(rng.normal(0, 6, (2_000_000, 5)) / 2)
    return _cut([rng.uniform(-1, 1, 6_000_000), np.prod(t, axis=1), t[:, 0] * t[:, 1],
                 1 - 10.0 ** rng.uniform(-16.5, 0, 3_000_000),
                 -1 + 10.0 ** rng.uniform(-16.5, 0, 3_000_000),
                 rng.uniform(-0.07, 0.07, 3_000_000),
                 rng.uniform(-1, 1, 1_000_000) * 10.0 ** rng.uniform(-300, 0, 1_000_000),
                 np.array([1.0, -1.0, 0.0, -0.0, np.nan, 0.5, -0.5, 1 - 2.0 ** -53,
                           -1 + 2.0 ** -53, np.nan, 1.0, 1.0])], cap)


def division_cases(perturb=0, cap=None):
    """The nine (a, b) families of test_batched_division_is_ieee: the three
    divisions of the sum-product pass (expm1's (r1 - t) / (6 - x t) ~ O(1),
    tanh's -t/(t+2) or 2/(t+2), (1+T)/(1-T) down to 2^-53), significands with
    long runs of ones / zeros (the hard cases of division), 1 / (1 - 2^-53)
    and quotients within 2^-39 ulp of a midpoint."""
    rng = np.random.default_rng(105 + abs(perturb))
    n = 3_000_000
    hard = (np.int64(0x3FF0000000000000) |
            (rng.integers(0, 2, n) * ((1 << 52) - 1) ^ rng.integers(0, 1 << 20, n))).view(np.float64)
    cases = [(rng.uniform(-2.2, -1.8, n), rng.uniform(5, 7, n)),
             (rng.uniform(0, 0.87, n), rng.uniform(1.13, 2, n)),
             (np.full(n, 2.0), 2 + np.exp(rng.uniform(1.8, 44, n))),
             (1 + rng.uniform(-1, 1, n), 1 - rng.uniform(-1, 1, n) * 10.0 ** -rng.uniform(0, 16, n)),
             (hard, np.roll(hard, 1)), (rng.uniform(1, 2, n), hard),
             # 1 / (1 - 2^-53) = 1 + 2^-53 + 2^-106...: just above a midpoint,
             # where the residual-corrected quotient alone rounds the wrong way
             (np.ones(n), np.full(n, 1 - 2.0 ** -53)),
             (1 + rng.integers(0, 1 << 12, n) * 2.0 ** -52,
              (np.int64(0x3FEFFFFFFFFFFFFF) - rng.integers(0, 1 << 8, n)).view(np.float64)),
             (1 + rng.uniform(-1, 1, n) * 2.0 ** -53 * rng.integers(0, 3, n),
              1 - rng.integers(0, 3, n) * 2.0 ** -53)]
    return [tuple(_cut(c, cap)) for c in cases]


# ---- tests/test_math.py ------------------------------------------------------------------

def check_pass_ratio_sets():
    rng = np.random.default_rng(14)
    return [rng.uniform(-1, 1, 400_000), np.tanh(rng.normal(0, 10, 400_000)),
            1 - 10.0 ** rng.uniform(-16, 0, 200_000), -1 + 10.0 ** rng.uniform(-16, 0, 200_000),
            np.array([1.0, -1.0, 0.0, -0.0, np.nan, 0.5, -0.5, 1 - 2.0 ** -53, -1 + 2.0 ** -53])]


def two_range_sets():
    """(far, mid) of test_two_range_tanh_matches_libm_near_one: |m| >= 16 and
    the specials beyond; |m| in [8, 16)"""
    rng = np.random.default_rng(21)
    far = np.concatenate([rng.uniform(16, 60, 400_000), -rng.uniform(16, 60, 400_000),
                          np.array([np.inf, -np.inf, 44.0, 38.0, 100.0, 1e300])])
    mid = rng.uniform(8, 16, 400_000) * rng.choice([-1.0, 1.0], 400_000)
    return far, mid


def table_log_sets():
    rng = np.random.default_rng(15)
    return [rng.uniform(-1, 1, 400_000), np.tanh(rng.normal(0, 10, 400_000)),
            1 - 10.0 ** rng.uniform(-16, 0, 200_000), -1 + 10.0 ** rng.uniform(-16, 0, 200_000),
            10.0 ** rng.uniform(-300, -1, 200_000),
            np.array([1.0, -1.0, 0.0, -0.0, np.nan, 0.5, -0.5, 1 - 2.0 ** -53, -1 + 2.0 ** -53])]


def batched_division_operands():
    """(m, T) of test_batched_divisions: bit messages with |m| <= 16 and open
    check operands, products of tanh(m/2) with |m| <= 16"""
    rng = np.random.default_rng(21)
    m = np.concatenate([rng.uniform(-16, 16, 600_000), rng.normal(0, 3, 600_000),
                        rng.uniform(-1, 1, 300_000) * 10.0 ** rng.uniform(-12, 0, 300_000)])
    t = np.tanh(rng.uniform(-8, 8, (1_200_000, 3)) / 1.0)
    T = (t[:, 0] * t[:, 1] * rng.choice([1.0, 0.5, 1e-3], t.shape[0])).astype(np.float64)
    T = np.concatenate([T, np.tanh(rng.uniform(-8, 8, 300_000))])
    return m, T


# ---- what the device tests add ---------------------------------------------------------------

def shuffled(*arrays, seed=7):
    """The arrays under one seeded permutation: cold-path operands and
    ordinary ones share waves."""
    p = np.random.default_rng(seed).permutation(arrays[0].size)
    out = [np.ascontiguousarray(a[p]) for a in arrays]
    return out[0] if len(out) == 1 else out


def pooled(sets, seed=7):
    """The sets as one shuffled array."""
    return shuffled(np.concatenate([np.asarray(s, np.float64).ravel() for s in sets]), seed=seed)


def whole_wave_cold():
    """Sets in which every operand of a wave takes the cold path, in order (not
    shuffled), four waves each:
      near1   T whose ratio (1+T)/(1-T) is within glibc's |q - 1| < 1/16 window
              and not 1: 192 packed ratios per wave, three passes of
              log_ratio_n_packed
      zeros   T = +-0 (q = 1: every lane reads the zero cell)
      edge    T = +-1 and NaN (every lane in ratio_fix_n)
      flagged the quotient 1 / (1 - 2^-53), which div_core flags on every lane"""
    n = 4 * WAVE
    rng = np.random.default_rng(23)
    near1 = rng.uniform(1e-3, 0.03, n) * rng.choice([-1.0, 1.0], n)
    zeros = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    edge = np.array([1.0, -1.0, np.nan])[np.arange(n) % 3]
    flagged = (np.ones(n), np.full(n, 1 - 2.0 ** -53))
    return dict(near1=near1, zeros=zeros, edge=edge, flagged=flagged)


def masked_operands(m, seed=11):
    """(m', mask) for tanh_half_n's masked overload: a tenth of the operands
    become structural zeros of either sign, and only those are masked (the
    form's contract).  Zeros elsewhere in m stay unmasked."""
    rng = np.random.default_rng(seed)
    mask = rng.random(m.size) < 0.1
    z = np.where(rng.random(m.size) < 0.5, 0.0, -0.0)
    return np.where(mask, z, m), mask.astype(np.float64)


def ulps(a, b):
    """Distance in units in the last place between two arrays of one float
    type, as integers; NaN against NaN is 0, +0 against -0 is 0."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b, a.dtype)
    it = np.int64 if a.dtype == np.float64 else np.int32
    top = np.int64(1) << (63 if a.dtype == np.float64 else 31)
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    if a.dtype == np.float64:
        # two's-complement wrap is what the ordering needs here
        with np.errstate(over="ignore"):
            ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
            ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
        d = np.abs(ia.astype(np.float64) - ib.astype(np.float64))
        exact = np.abs(ia - ib)
        d = np.where(d < 2.0 ** 62, exact.astype(np.float64), d)
    else:
        ia = np.where(ia < 0, -top - ia, ia)
        ib = np.where(ib < 0, -top - ib, ib)
        d = np.abs(ia - ib).astype(np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0.0, np.where(one_nan, np.inf, d))


def same_bits(a, b):
    """Elementwise: equal as bit patterns (so the sign of zero counts), or both NaN."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b, a.dtype)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


# ---- the pools the device tests upload (and the host runs first) ---------------------------------

def tanh_pool():
    return pooled(tanh_half_sets(GPU_CAP))


def ratio_pool():
    return pooled(log_ratio_sets(GPU_CAP))


def division_pool():
    """(a, b): the nine families, GPU_CAP pairs each, under one permutation"""
    cases = division_cases(0, GPU_CAP)
    return shuffled(np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases]))


def fast_tanh_pool():
    """precision 3's tanh operands: test_math.py's inputs and both two-range sets"""
    far, mid = two_range_sets()
    return pooled(inputs(22) + [far, mid])


def fast_small_pool():
    """the batched single-range form's domain, |m| <= 8"""
    m, _ = batched_division_operands()
    return shuffled(m[np.abs(m) <= 8.0])


def fast_open_pool():
    """the open table log's domain, |T| <= tanh(8): test_batched_divisions'
    operands and the table log's vanishing T (10^-300 .. 0.1, either sign),
    whose ratios next to 1 need the IEEE quotient (ldpc_math.hpp ratio_fast)"""
    _, T = batched_division_operands()
    tiny = table_log_sets()[4]
    T = np.concatenate([T, tiny, -tiny])
    return shuffled(T[np.abs(T) <= np.tanh(8.0)])


def fast_division_pool():
    """(a, b) of the two divisions div_fast_n serves, formed from
    test_batched_divisions' operands: -t / (t + 2) with t = expm1(-|m|), and
    (1 + T) / (1 - T)"""
    m, T = batched_division_operands()
    t = np.expm1(-np.abs(m))
    T = T[np.abs(T) <= np.tanh(8.0)]
    return shuffled(np.concatenate([-t, 1.0 + T]), np.concatenate([t + 2.0, 1.0 - T]))


# ---- precision 3's bounds (ldpc_device.hpp) ----------------------------------------

def fast_tanh_errors(m, z, ref):
    """max ulp of z against glibc's ref, overall / for |m| >= 2 / for |m| >= 16"""
    u = ulps(z, ref)
    a = np.abs(m)
    return float(u.max()), float(u[a >= 2.0].max()), float(u[a >= 16.0].max())


def assert_fast_tanh(m, z, ref):
    """tanh_half at precision 3: within 3 ulp of glibc, within 1 ulp for
    |m| >= 2, glibc's double for |m| >= 16"""
    e_all, e_2, e_16 = fast_tanh_errors(m, z, ref)
    assert e_all <= 3, e_all
    assert e_2 <= 1, e_2
    assert e_16 == 0, e_16
    return e_all, e_2, e_16
