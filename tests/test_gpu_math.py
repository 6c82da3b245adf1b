"""The decode kernels' arithmetic on the device, operand by operand.

ldpc_math_probe evaluates one function through the calls the kernels make
(csrc/ldpc_probe.hip), one group of three operands per lane, so every
wave-uniform cold branch runs with 63 lanes that did not ask for it and every
batched division starts from the device's own reciprocal seed.  The operands
are the pools of tests/math_sets.py: the host tests' sets, capped at 2^20
each and shuffled, which tests/test_math_sets_host.py passes through the same
code on the host first; plus sets in which a whole wave is cold.

  precisions 0 and 2   glibc's double, as bit patterns (NaN == NaN, the sign
                       of zero counts); divisions equal IEEE division
  precision 3          the bounds of csrc/ldpc_device.hpp and DESIGN section 5
                       against glibc
  precision 1          what follows from the definitions (edges, oddness,
                       range, monotonicity) and an accuracy no more than one
                       ulp worse than the host's tanhf / logf against the
                       correctly rounded value

The reference values are the host libm's, through the oracle's elementwise
helpers.  Every call writes into a buffer with a canary behind its n elements.
The maxima printed here are recorded in profiles/round23/device_math.txt."""
import numpy as np
import pytest

import ldpc_ece535a as L
import math_sets as ms
from math_probe import Probe
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C = L._capi


@pytest.fixture(scope="module")
def probe():
    p = Probe()
    yield p
    p.close()


@pytest.fixture(scope="module")
def pools():
    """the operand pools and glibc's values on them, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "tanh":
                m = ms.tanh_pool()
                cache[name] = (m, orc.tanh_half(m))
            elif name == "ratio":
                T = ms.ratio_pool()
                cache[name] = (T, orc.log_ratio(T))
            elif name == "division":
                a, b = ms.division_pool()
                cache[name] = (a, b, orc.div(a, b))
            elif name == "cold":
                cache[name] = ms.whole_wave_cold()
        return cache[name]
    return get


def _all_same(z, ref, what):
    same = ms.same_bits(z, ref)
    assert same.all(), "%s: %d of %d differ, first at %d: %r vs glibc %r" % (
        what, (~same).sum(), same.size, np.flatnonzero(~same)[0], z[~same][:4], ref[~same][:4])


def _within(u, bound, what, x, z, ref):
    """max ulp printed, then asserted, with the worst operand in the message"""
    i = int(np.argmax(u))
    print("%s max ulp: %g" % (what, u[i]))
    assert u[i] <= bound, "%s: %g ulp at operand %r: %r vs glibc %r; %d operands beyond %g ulp" % (
        what, u[i], x[i], z[i], ref[i], int((u > bound).sum()), bound)


# ---- the seam itself ------------------------------------------------------------------------------

def test_probe_refuses_bad_arguments(probe):
    d = torch.zeros(6, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = d.data_ptr()
    bad = [dict(fn=C.PROBE_TANH_HALF, precision=0, d_a=p, n=4, d_out=p),            # not a multiple of 3
           dict(fn=C.PROBE_TANH_HALF, precision=0, d_a=p, n=-3, d_out=p),
           dict(fn=C.PROBE_TANH_HALF, precision=4, d_a=p, n=3, d_out=p),
           dict(fn=10, precision=0, d_a=p, n=3, d_out=p),
           dict(fn=-1, precision=0, d_a=p, n=3, d_out=p),
           dict(fn=C.PROBE_TANH_HALF, precision=0, d_a=None, n=3, d_out=p),
           dict(fn=C.PROBE_TANH_HALF, precision=0, d_a=p, n=3, d_out=None),
           dict(fn=C.PROBE_DIV3, precision=0, d_a=p, n=3, d_out=p),                 # needs d_b
           dict(fn=C.PROBE_TANH_HALF_MASKED, precision=0, d_a=p, n=3, d_out=p),
           dict(fn=C.PROBE_TANH_HALF_MASKED, precision=2, d_a=p, n=3, d_out=p, d_b=p),  # 0 only
           dict(fn=C.PROBE_CHECK_MSG_PACKED, precision=3, d_a=p, n=3, d_out=p),
           dict(fn=C.PROBE_TANH_HALF_SMALL3, precision=0, d_a=p, n=3, d_out=p),
           dict(fn=C.PROBE_CHECK_MSG_OPEN3, precision=1, d_a=p, n=3, d_out=p),
           dict(fn=C.PROBE_DIV1, precision=3, d_a=p, n=3, d_out=p, d_b=p),
           dict(fn=C.PROBE_DIV3, precision=1, d_a=p, n=3, d_out=p, d_b=p)]
    for kw in bad:
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL: math probe"):
            probe.dec.math_probe(**kw)
    probe.dec.math_probe(C.PROBE_TANH_HALF, 0, None, 0, None)   # nothing to do
    probe.dec.synchronize()
    assert (d.cpu().numpy() == 0).all()


# ---- precisions 0 and 2: glibc, bit for bit --------------------------------------------------------

@pytest.mark.parametrize("prec", [C.PREC_F64, C.PREC_F64_LIBM])
def test_tanh_half_is_glibc(probe, pools, prec):
    m, ref = pools("tanh")
    _all_same(probe(C.PROBE_TANH_HALF, prec, m), ref, "tanh_half precision %d" % prec)


def test_tanh_half_masked_is_glibc(probe, pools):
    """the masked overload: every unmasked lane is glibc's value (exact zeros
    among them), every masked lane returns the zero it was given"""
    m, ref = pools("tanh")
    mm, mask = ms.masked_operands(m)
    z = probe(C.PROBE_TANH_HALF_MASKED, C.PREC_F64, mm, mask)
    free = mask == 0
    assert (mm[free] == 0).sum() >= 2   # unmasked zeros take the cold path
    _all_same(z[free], ref[free], "masked tanh_half, unmasked lanes")
    _all_same(z[~free], mm[~free], "masked tanh_half, masked lanes")


@pytest.mark.parametrize("prec", [C.PREC_F64, C.PREC_F64_LIBM])
def test_check_msg_is_glibc(probe, pools, prec):
    T, ref = pools("ratio")
    _all_same(probe(C.PROBE_CHECK_MSG, prec, T), ref, "check_msg precision %d" % prec)
    for name in ("near1", "zeros", "edge"):
        t = pools("cold")[name]
        _all_same(probe(C.PROBE_CHECK_MSG, prec, t), orc.log_ratio(t),
                  "check_msg precision %d, whole waves of %s" % (prec, name))


@pytest.mark.parametrize("fn", [C.PROBE_CHECK_MSG_PACKED, C.PROBE_CHECK_MSG_PACKED_LEAN],
                         ids=["packed", "lean"])
def test_packed_check_msg_is_glibc(probe, pools, fn):
    """log_ratio_n_packed on |T| <= 1 and NaN; whole waves of near-1 ratios
    (192 packed cells: three dense passes), of +-0 (every lane on the zero
    cell) and of +-1 / NaN; and a last, partly filled block"""
    T, ref = pools("ratio")
    _all_same(probe(fn, C.PREC_F64, T), ref, "packed check_msg")
    for name in ("near1", "zeros", "edge"):
        t = pools("cold")[name]
        _all_same(probe(fn, C.PREC_F64, t), orc.log_ratio(t), "packed, whole waves of " + name)
    t = np.concatenate([pools("cold")["near1"], T[:3 * 37]])   # 256 + 37 groups
    _all_same(probe(fn, C.PREC_F64, t), orc.log_ratio(t), "packed, a partly filled block")


@pytest.mark.parametrize("fn", [C.PROBE_DIV1, C.PROBE_DIV2, C.PROBE_DIV3], ids=["1", "2", "3"])
def test_division_is_ieee(probe, pools, fn):
    """div_n<k> from the device's reciprocal seed: a / b on the nine families
    of test_batched_division_is_ieee, and on whole waves of the flagged
    quotient 1 / (1 - 2^-53)"""
    a, b, ref = pools("division")
    _all_same(probe(fn, C.PREC_F64, a, b), ref, "div_n")
    fa, fb = pools("cold")["flagged"]
    _all_same(probe(fn, C.PREC_F64, fa, fb), orc.div(fa, fb), "div_n, whole waves flagged")
    if fn == C.PROBE_DIV3:   # mode 2 divides as mode 0 does
        _all_same(probe(fn, C.PREC_F64_LIBM, a[:30000], b[:30000]), ref[:30000], "div_n, mode 2")


# ---- precision 3: the project's bounds ------------------------------------------------------------------

def test_fast_tanh_half_bounds(probe):
    """tanh_half_acc: within 3 ulp of glibc, within 1 ulp for |m| >= 2, glibc's
    double for |m| >= 16"""
    m = ms.fast_tanh_pool()
    z = probe(C.PROBE_TANH_HALF, C.PREC_F64_FAST, m)
    ref = orc.tanh_half(m)
    print("precision 3 tanh_half max ulp: all %g, |m| >= 2 %g, |m| >= 16 %g"
          % ms.fast_tanh_errors(m, z, ref))
    ms.assert_fast_tanh(m, z, ref)
    assert ms.same_bits(z[m == 0], m[m == 0]).all()


def test_fast_check_msg_within_1ulp(probe):
    T = ms.pooled(ms.table_log_sets())
    z, ref = probe(C.PROBE_CHECK_MSG, C.PREC_F64_FAST, T), orc.log_ratio(T)
    _within(ms.ulps(z, ref), 1, "precision 3 check_msg", T, z, ref)


def test_fast_batched_tanh_within_3ulp(probe):
    """the small-code route's batched single-range form on its domain, |m| <= 8"""
    m = ms.fast_small_pool()
    z, ref = probe(C.PROBE_TANH_HALF_SMALL3, C.PREC_F64_FAST, m), orc.tanh_half(m)
    _within(ms.ulps(z, ref), 3, "precision 3 tanh_half_small_n", m, z, ref)


def test_fast_batched_log_within_3ulp(probe):
    """the small-code route's batched open table log on its domain, |T| <= tanh(8)"""
    T = ms.fast_open_pool()
    z, ref = probe(C.PROBE_CHECK_MSG_OPEN3, C.PREC_F64_FAST, T), orc.log_ratio(T)
    _within(ms.ulps(z, ref), 3, "precision 3 log_ratio_tab_open_n", T, z, ref)


def test_fast_division_within_1ulp(probe):
    a, b = ms.fast_division_pool()
    z, ref = probe(C.PROBE_DIV3, C.PREC_F64_FAST, a, b), orc.div(a, b)
    _within(ms.ulps(z, ref), 1, "precision 3 div_fast_n", a / b, z, ref)


# ---- precision 1 -------------------------------------------------------------------------------------------

def _f32_operands():
    rng = np.random.default_rng(41)
    n = 1 << 18
    m = np.concatenate([rng.uniform(-30, 30, n), rng.normal(0, 8, n), rng.uniform(-2, 2, n),
                        rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-20, 0, n)]).astype(np.float32)
    t = np.tanh(rng.normal(0, 6, (n, 3)) / 2)
    T = np.concatenate([rng.uniform(-1, 1, n), t[:, 0] * t[:, 1], t[:, 0] * t[:, 1] * t[:, 2],
                        rng.uniform(-0.07, 0.07, n), 1 - 10.0 ** rng.uniform(-7, 0, n),
                        -1 + 10.0 ** rng.uniform(-7, 0, n)]).astype(np.float32)
    return ms.shuffled(m), ms.shuffled(T[np.abs(T) < 1])


def test_f32_properties(probe):
    F = C.PREC_F32
    m, _ = _f32_operands()
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    z = probe(C.PROBE_TANH_HALF, F, edge)
    assert ms.same_bits(z[:4], np.array([0.0, -0.0, 1.0, -1.0], np.float32)).all()
    assert np.isnan(z[4])
    z = probe(C.PROBE_TANH_HALF, F, m)
    assert (np.abs(z) <= 1).all()
    assert ms.same_bits(probe(C.PROBE_TANH_HALF, F, -m), -z).all()   # odd, bit for bit
    sweep = np.sort(np.concatenate([m, np.linspace(-40, 40, 1 << 18).astype(np.float32)]))
    zs = probe(C.PROBE_TANH_HALF, F, sweep)
    assert (np.diff(zs) >= 0).all()
    e = probe(C.PROBE_CHECK_MSG, F, np.array([1.0, -1.0, 0.0, -0.0], np.float32))
    assert e[0] == np.inf and e[1] == -np.inf and e[2] == 0 and e[3] == 0


def test_f32_accuracy_against_the_host(probe):
    """Device tanhf(m / 2) and logf against the correctly rounded float of the
    long double value, in ulp, beside the same error of the host's tanhf /
    logf on the same operands.  The project fixes no bound for them; a
    faithful implementation may choose the other neighbour in the last place,
    so the device may be one ulp worse than the host and no more."""
    assert np.finfo(np.longdouble).nmant >= 63
    F = C.PREC_F32
    m, T = _f32_operands()
    ref = np.tanh(m.astype(np.longdouble) / 2).astype(np.float32)
    dev = ms.ulps(probe(C.PROBE_TANH_HALF, F, m), ref).max()
    host = ms.ulps(orc.tanh_half_f32(m), ref).max()
    print("precision 1 tanh_half max ulp: device %g, host %g" % (dev, host))
    assert dev <= host + 1
    # only logf is measured: q is formed in float here, as the kernel forms it
    q = ((np.float32(1) + T) / (np.float32(1) - T)).astype(np.float32)
    assert np.isfinite(q).all() and (q > 0).all()
    ref = np.log(q.astype(np.longdouble)).astype(np.float32)
    dev = ms.ulps(probe(C.PROBE_CHECK_MSG, F, T), ref).max()
    host = ms.ulps(orc.log_f32(q), ref).max()
    print("precision 1 check_msg (logf) max ulp: device %g, host %g" % (dev, host))
    assert dev <= host + 1
