"""CPU: rate matching's host entry points (ldpc_plan_rate_match, ldpc_rate_match,
ldpc_rate_recover: csrc/ldpc_rate_match.cc, the index functions the kernels
run) against the numpy restatement (tests/rate_match_ref.py): the literal walk
of the buffer, the closed form, and the combine in sample order."""
import numpy as np
import pytest

import rate_match_cases as rc
import rate_match_ref as rm

TINY = 2.0 ** -100


def _random_pattern(rng):
    """A legal pattern and 1..4 legal transmissions on a random shape."""
    N = int(rng.integers(3, 200))
    M = int(rng.integers(1, N - 1))
    K = N - M
    filler = int(rng.integers(0, K + 1)) if rng.random() < 0.7 else 0
    punct = int(rng.integers(0, K - filler + 1)) if rng.random() < 0.7 else 0
    lo = max(K - punct, filler + 1)
    ncb = int(rng.integers(lo, N - punct + 1))
    if ncb == N - punct and rng.random() < 0.5:
        ncb = 0
    S = (ncb or N - punct) - filler
    tx = [(int(rng.integers(0, ncb or N - punct)), int(rng.integers(1, min(16 * S, 3 * S + 8) + 1)))
          for _ in range(int(rng.integers(1, 5)))]
    return M, N, (punct, filler, ncb), tx


def test_closed_form_is_the_literal_walk():
    """20 000 seeded random patterns, numpy against numpy."""
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(20000):
        M, N, pat, tx = _random_pattern(rng)
        k0, E = tx[0]
        np.testing.assert_array_equal(rm.closed(M, N, *pat, k0, E), rm.walk(M, N, *pat, k0, E),
                                      err_msg=str((M, N, pat, k0, E)))


def test_plan_against_both_restatements():
    from ldpc_ece535a import _capi
    rng = np.random.Generator(np.random.PCG64(12))
    for _ in range(3000):
        M, N, pat, tx = _random_pattern(rng)
        plan = _capi.plan_rate_match(M, N, *pat, tx)
        what = str((M, N, pat, tx))
        assert plan["total"] == sum(e for _, e in tx), what
        np.testing.assert_array_equal(plan["col"], rm.columns(M, N, pat, tx), err_msg=what)
        np.testing.assert_array_equal(
            plan["col"], np.concatenate([rm.walk(M, N, *pat, k0, e) for k0, e in tx]), err_msg=what)
        np.testing.assert_array_equal(plan["count"], rm.counts(M, N, pat, tx), err_msg=what)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_counts_of_the_shared_cases(name):
    """count sums to the samples sent, and no sample lands on a punctured
    column, a filler or a column outside the buffer."""
    from ldpc_ece535a import _capi
    c = rc.CASES[name]
    M, N, (punct, filler, ncb) = c["M"], c["N"], c["pattern"]
    K = N - M
    plan = _capi.plan_rate_match(M, N, punct, filler, ncb, c["tx"])
    count = plan["count"]
    assert plan["total"] == rc.total(c) and count[count > 0].sum() == plan["total"]
    pos = np.where(np.arange(N) >= M, np.arange(N) - M, np.arange(N) + K)
    fill = (pos >= K - filler) & (pos < K)
    assert ((count == -1) == fill).all()
    outside = (pos < punct) | (pos >= punct + (ncb or N - punct))
    assert (count[outside & ~fill] == 0).all()
    np.testing.assert_array_equal(plan["col"], np.concatenate(
        [rm.walk(M, N, punct, filler, ncb, k0, e) for k0, e in c["tx"]]))


def test_repetition_gives_one_two_and_three_terms():
    from ldpc_ece535a import _capi
    seen = set()
    for name in ("c", "c3"):
        c = rc.CASES[name]
        seen |= set(_capi.plan_rate_match(c["M"], c["N"], *c["pattern"], c["tx"])["count"].tolist())
    assert {-1, 0, 1, 2, 3} <= seen


def test_identity_is_the_column_permutation():
    from ldpc_ece535a import _capi
    M, N = 324, 648
    plan = _capi.plan_rate_match(M, N, 0, 0, 0, [(0, N)])
    np.testing.assert_array_equal(plan["col"], np.r_[M:N, 0:M])
    assert (plan["count"] == 1).all()
    rng = np.random.Generator(np.random.PCG64(13))
    bits = rng.integers(0, 2, (5, N), np.uint8)
    np.testing.assert_array_equal(_capi.rate_match(M, N, 0, 0, 0, 0, N, bits),
                                  bits[:, np.r_[M:N, 0:M]])
    rx = rc.plant_special(rng.standard_normal((5, N)).astype(np.float32))
    y = _capi.rate_recover(M, N, 0, 0, 0, [(0, N)], rx)
    want = np.empty_like(rx)
    want[:, np.r_[M:N, 0:M]] = rx          # -(-(x * 1)) is x, NaN and -0.0 included
    assert rm.bits_equal(y, want)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_host_select_and_combine(name):
    """ldpc_rate_match and ldpc_rate_recover against numpy, bit for bit, with
    +-inf, +-0.0 and NaN planted, at both polarities, at a stride beyond sum E,
    and with 0.0 for the unreceived columns."""
    from ldpc_ece535a import _capi
    c = rc.CASES[name]
    M, N, pat, tx = c["M"], c["N"], c["pattern"], c["tx"]
    rng = np.random.Generator(np.random.PCG64(14))
    B = 6
    bits = rng.integers(0, 2, (B, N), np.uint8)
    dirty = np.where(bits == 1, 0x03, 0xFE).astype(np.uint8)   # bit 0 alone counts
    for k0, E in tx:
        want = bits[:, rm.closed(M, N, *pat, k0, E)]
        np.testing.assert_array_equal(_capi.rate_match(M, N, *pat, k0, E, bits), want)
        np.testing.assert_array_equal(_capi.rate_match(M, N, *pat, k0, E, dirty), want)
    rx = rc.plant_special(rng.standard_normal((B, rc.total(c))).astype(np.float32))
    for pol, un, pad in ((1.0, TINY, 0), (-1.0, TINY, 5), (1.0, 0.0, 0), (-2.5, -3.0, 1)):
        got = _capi.rate_recover(M, N, *pat, tx, rc.strided(rx, pad), polarity=pol,
                                 unreceived_lci=un, rx_stride=rx.shape[1] + pad, B=B)
        want = -rm.recover(M, N, pat, tx, rx, pol, un)
        assert rm.bits_equal(got, want), (pol, un, pad)
    fill = rm.filler_columns(M, N, pat)
    assert (got[:, fill] == -np.inf).all()


REFUSALS = [
    ((-1, 0, 0), [(0, 4)], r"punct must be >= 0 \(got -1\)"),
    ((0, -2, 0), [(0, 4)], r"filler must be >= 0 \(got -2\)"),
    ((0, 0, -3), [(0, 4)], r"ncb must be >= 0.*\(got -3\)"),
    ((7, 2, 0), [(0, 4)], r"punct must be <= K - filler = 6 \(got 7\)"),
    ((0, 0, 7), [(0, 4)], r"punct \+ ncb must be in \[K, N\] = \[8, 12\]; ncb \(got 7\)"),
    ((2, 0, 11), [(0, 4)], r"punct \+ ncb must be in \[K, N\].*ncb \(got 11\)"),
    ((0, 8, 8), [(0, 4)], r"S = ncb - filler must be >= 1; S \(got 0\)"),
    ((0, 0, 0), [(12, 4)], r"k0 must be in \[0, ncb = 12\) \(got 12\)"),
    ((0, 0, 0), [(-1, 4)], r"k0 must be in \[0, ncb = 12\) \(got -1\)"),
    ((0, 0, 0), [(0, 0)], r"E must be in \[1, 16 S = 192\] \(got 0\)"),
    ((0, 0, 0), [(0, 193)], r"E must be in \[1, 16 S = 192\] \(got 193\)"),
    ((0, 0, 0), [], r"n_tx must be in \[1, 4\].*\(got 0\)"),
    ((0, 0, 0), [(0, 4)] * 5, r"n_tx must be in \[1, 4\].*\(got 5\)"),
]


@pytest.mark.parametrize("pattern,tx,message", REFUSALS)
def test_refusals_name_the_value(pattern, tx, message):
    """On a 4 x 12 code (K = 8)."""
    from ldpc_ece535a import _capi
    with pytest.raises(_capi.LdpcError, match="LDPC_EINVAL.*" + message):
        _capi.plan_rate_match(4, 12, *pattern, tx)


def test_limits_are_accepted():
    from ldpc_ece535a import _capi
    assert _capi.plan_rate_match(4, 12, 0, 0, 0, [(11, 192)] * 4)["total"] == 768
    assert _capi.plan_rate_match(4, 12, 6, 2, 3, [(0, 1)])["total"] == 1    # punct = K - filler
    assert _capi.plan_rate_match(4, 12, 0, 7, 8, [(0, 16)])["total"] == 16  # S = 1


def test_combine_refusals():
    from ldpc_ece535a import _capi
    rx = np.ones((1, 4), np.float32)
    with pytest.raises(_capi.LdpcError, match="unreceived_lci must not be NaN"):
        _capi.rate_recover(4, 12, 0, 0, 0, [(0, 4)], rx, unreceived_lci=float("nan"))
    with pytest.raises(_capi.LdpcError, match="rx_stride >= the sum of E"):
        _capi.rate_recover(4, 12, 0, 0, 0, [(0, 4)], rx, rx_stride=3, B=1)
    with pytest.raises(_capi.LdpcError, match="input shorter than the frames read"):
        _capi.rate_recover(4, 12, 0, 0, 0, [(0, 4)], rx, rx_stride=4, B=2)


def test_a_start_inside_the_fillers_is_accepted():
    """Case (d2): the fillers are buffer offsets [230, 270); k0 = 250 starts at
    offset 270, as k0 = 270 does."""
    from ldpc_ece535a import _capi
    c = rc.CASES["d2"]
    M, N, pat = c["M"], c["N"], c["pattern"]
    K, _, _, fs, fe = rm.resolve(M, N, *pat)
    assert (fs, fe) == (230, 270) and fs <= 250 < fe
    inside = _capi.plan_rate_match(M, N, *pat, [(250, 100)])["col"]
    np.testing.assert_array_equal(inside, _capi.plan_rate_match(M, N, *pat, [(270, 100)])["col"])
    np.testing.assert_array_equal(inside, rm.walk(M, N, *pat, 250, 100))
    assert inside[0] == rm.col_of_pos(M, N, pat[0] + 270)
