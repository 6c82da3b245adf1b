"""Host: tests/channel_ref.py pinned without a GPU -- Philox4x32-10 to the
Random123 known answers, the uniform maps at their edges, the extreme draws
that tests/test_gpu_channel.py names, and a demonstration that the comparison
the GPU test makes fails for each fault it is there to catch."""
import math

import numpy as np
import pytest

import channel_ref as cr

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = cr.philox4x32_10(*ctr, *key)
    assert " ".join("%08x" % int(w[0]) for w in got) == want


def test_philox_is_vectorised():
    """Rows of an array draw equal the scalar draws, the third known answer among them."""
    ctr, key, want = KAT[2]
    c = [np.array([0, v, 0xFFFFFFFF], np.uint64) for v in ctr]
    k = [np.array([0, v, 0xFFFFFFFF], np.uint64) for v in key]
    got = np.stack(cr.philox4x32_10(*c, *k), axis=1)
    for row, (_, _, w) in zip(got, (KAT[0], KAT[2], KAT[1])):
        assert " ".join("%08x" % int(v) for v in row) == w


def test_draw_layout():
    """Counter (lo, hi, stream, 0x2545F491), key (seed lo, seed hi)."""
    seed = 0x0123456789ABCDEF
    ctr = np.array([0, 5, (7 << 32) | 9], np.uint64)
    got = cr.draw(3, 2, seed, ctr=ctr)
    for row, c in zip(got, ctr):
        c = int(c)
        want = cr.philox4x32_10(c & 0xFFFFFFFF, c >> 32, 2, 0x2545F491, 0x89ABCDEF, 0x01234567)
        assert [int(v) for v in row] == [int(w[0]) for w in want]
    assert (cr.draw(6, 2, seed)[5] == got[1]).all()      # the default counters are 0, 1, ...


def test_random_bits_layout():
    w = cr.draw(3, 1, 77)
    b = cr.random_bits(10, 77)
    assert b.dtype == np.uint8 and b.shape == (10,)
    assert [int(v) for v in b] == [int(w[i >> 2, i & 3]) >> 31 for i in range(10)]
    assert cr.random_bits(0, 77).size == 0
    # a prefix of a longer draw: the tail of n % 4 != 0 takes the same counter
    for n in (1, 2, 3, 5):
        assert (cr.random_bits(n, 77) == b[:n]).all()
    big = cr.random_bits(1 << 16, 77)
    assert abs(big.mean() - 0.5) < 4 * 0.5 / math.sqrt(1 << 16)


def test_uniform_maps_at_their_edges():
    """u1 in (0, 1], u2 in [0, 1]; fl(x) rounds to nearest even, so the top
    128 words give fl(x) = 2^32 and u1 = u2 = 1."""
    x = np.array([0, 1, 0x2C, 0x7FFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFF2, 0xFFFFFFFF], np.uint64)
    words = np.stack([x, x, x, x], axis=1)
    u1, u2 = cr.uniforms_of(words)
    assert (u1[:, 0] == u1[:, 1]).all() and (u2[:, 0] == u2[:, 1]).all()
    two32 = 2.0 ** 32
    assert list(u2[:, 0].astype(np.float64) * two32) == [0, 1, 44, 2.0 ** 31, two32 - 256, two32,
                                                         two32, two32]
    # 0xFFFFFF7F rounds down to 2^32 - 256, whose successor + 1 rounds back to it
    assert list(u1[:, 0].astype(np.float64) * two32) == [1, 2, 45, 2.0 ** 31, two32 - 256, two32,
                                                         two32, two32]
    assert u1.min() > 0 and u1.max() == 1 and u2.max() == 1


def test_normals_sample_order_and_bound():
    n = 4096
    words = cr.draw(n // 4, 2, 11)
    u1, u2 = cr.uniforms_of(words)
    z = cr.normals_f64(n, 11).reshape(-1, 4)
    r = np.sqrt(-2 * np.log(u1.astype(np.float64)))
    th = 2 * np.pi * u2.astype(np.float64)
    want = np.stack([r[:, 0] * np.cos(th[:, 0]), r[:, 0] * np.sin(th[:, 0]),
                     r[:, 1] * np.cos(th[:, 1]), r[:, 1] * np.sin(th[:, 1])], axis=1)
    np.testing.assert_allclose(z, want, rtol=0, atol=1e-14)
    assert np.abs(z).max() <= cr.BOUND
    # the quadrant reduction: exact zeros and ones where 2 u2 is a multiple of 1/2
    s, c = cr._sincospi(np.array([0.0, 0.5, 1.0, 1.5, 2.0]))
    assert list(s) == [0, 1, 0, -1, 0] and list(c) == [1, 0, -1, 0, 1]
    # the largest radius: x = 0
    zero = np.zeros((1, 4), np.uint64)
    assert cr.normals_of(zero)[0] == pytest.approx(cr.BOUND, rel=1e-15)
    assert cr.BOUND == pytest.approx(6.6604, abs=1e-4)


def test_normals_statistics():
    z = cr.normals_f64(1 << 18, 5)
    n = z.size
    assert abs(z.mean()) < 5 / math.sqrt(n) and abs(z.std() - 1) < 5 / math.sqrt(2 * n)
    assert abs((z ** 4).mean() - 3) < 5 * math.sqrt(96 / n)


# The extreme draws of tests/test_gpu_channel.py, re-derived: (seed, counter, word index, word)
EXTREMES = {
    "u1_is_one": (235, 16976, 0, 0xFFFFFFF2),
    "u1_small": (118, 212107, 0, 0x2C),
    "u2_is_one": (143, 14990, 1, 0xFFFFFFD3),
}


def test_extreme_draws():
    for seed, ctr, k, word in EXTREMES.values():
        assert int(cr.draw(ctr + 1, 2, seed)[ctr, k]) == word
    seed, ctr, _, _ = EXTREMES["u1_is_one"]
    z = cr.normals_f64(4 * ctr + 4, seed)
    assert (z[4 * ctr:4 * ctr + 2] == 0).all() and (z[4 * ctr + 2:] != 0).all()
    seed, ctr, _, _ = EXTREMES["u1_small"]
    z = cr.normals_f64(4 * ctr + 4, seed)
    assert math.hypot(z[4 * ctr], z[4 * ctr + 1]) == pytest.approx(6.06, abs=5e-3)
    seed, ctr, _, _ = EXTREMES["u2_is_one"]
    z = cr.normals_f64(4 * ctr + 4, seed)
    u1, u2 = cr.uniforms(4 * ctr + 4, seed)
    assert u2[ctr, 0] == 1.0
    assert z[4 * ctr + 1] == 0 and z[4 * ctr] == math.sqrt(-2 * math.log(float(u1[ctr, 0])))


def test_ulp_error():
    ref = np.array([1.0, 1.0, -3.0, 0.0, 2.0 ** -14])
    got = np.array([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -3.0, 0.0, 2.0 ** -14 * (1 + 2.0 ** -22)],
                   np.float32)
    assert list(cr.ulp_error(got, ref)) == [1.0, 0.5, 0.0, 0.0, 2.0]
    assert cr.ulp_error(np.float32(1e-30), 0.0) > 1e9


# ---- the comparison of the GPU test fails for every fault it is there to catch ------

N, SEED = 4096, 0x0000000300000007
LIMIT = cr.ULP_LIMIT


def _model(words, bits, lanes=(0, 1, 2, 3)):
    """A sigma = 2^40 run of a kernel that draws `words` and is otherwise
    exact: its deviates are the float64 ones rounded to float."""
    n_dev = cr.normals_of(words).reshape(-1, 4)[:, list(lanes)].reshape(-1).astype(np.float32)
    return cr.compose(bits, cr.SIGMA_BIG, n_dev[:bits.size])


def _words(**kw):
    return cr.draw(N // 4, kw.pop("stream", 2), kw.pop("seed", SEED), **kw)


def test_comparison_passes_for_the_exact_model():
    bits = cr.random_bits(N, 1)
    res = cr.check_scaled_run(_model(_words(), bits), cr.normals_f64(N, SEED), 0.5)
    assert max(res["max_ulp_by_position"]) <= 0.5
    ok = res["big"]
    assert (res["n_dev"][ok] == cr.normals_f64(N, SEED).astype(np.float32)[ok]).all()


FAULTS = {
    "sin and cos swapped": dict(lanes=(1, 0, 3, 2)),
    "the sin / cos of the two pairs exchanged": dict(lanes=(0, 3, 2, 1)),
    "u1 and u2 swapped": dict(perm=(1, 0, 3, 2)),
    "u2 exchanged between the pairs": dict(perm=(0, 3, 2, 1)),
    "stream 1 used for the noise": dict(stream=1),
    "seed high word dropped": dict(seed=SEED & 0xFFFFFFFF),
    "seed low word dropped": dict(seed=SEED >> 32 << 32),
    "counter i instead of i >> 2": dict(ctr=4 * np.arange(N // 4, dtype=np.uint64)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_comparison_catches(fault):
    kw = dict(FAULTS[fault])
    lanes = kw.pop("lanes", (0, 1, 2, 3))
    perm = kw.pop("perm", (0, 1, 2, 3))
    bits = cr.random_bits(N, 1)
    out = _model(_words(**kw)[:, list(perm)], bits, lanes)
    with pytest.raises(AssertionError, match="samples beyond"):
        cr.check_scaled_run(out, cr.normals_f64(N, SEED), LIMIT)


def test_comparison_catches_a_wrong_tail():
    """n % 4 != 0: the last counter's samples taken from the next counter."""
    n = N - 1
    bits = cr.random_bits(n, 1)
    words = _words()
    words[-1] = cr.draw(N // 4 + 1, 2, SEED)[-1]
    with pytest.raises(AssertionError, match="counter %d" % (N // 4 - 1)):
        cr.check_scaled_run(_model(words, bits), cr.normals_f64(n, SEED), LIMIT)


def test_composition_catches_a_fused_multiply_add():
    """fl(s + sigma * n) in one rounding differs from the two-rounding form on
    a share of samples large enough that a 4096-sample draw shows it."""
    bits = cr.random_bits(N, 1)
    n_dev = cr.normals_f64(N, SEED).astype(np.float32)
    sigma = np.float32(0.7)
    fused = (cr.bpsk(bits).astype(np.float64) + np.float64(sigma) * n_dev.astype(np.float64))
    assert (fused.astype(np.float32) != cr.compose(bits, sigma, n_dev)).sum() > 40
