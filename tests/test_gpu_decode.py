"""GPU parity: the HIP decode path (through the C ABI) against the golden
fixtures written by the C oracle (tests/golden/make_golden.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    import ldpc_ece535a
    return ldpc_ece535a.Decoder()  # default H, reordered like the block


@pytest.fixture(scope="module")
def dec_by_schedule():
    import ldpc_ece535a
    out = {}
    for sched in (1, 2):
        d = ldpc_ece535a.Decoder()
        d.set_schedule(sched)
        out[sched] = d
    return out


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("prec", [0, 2, 3])
@pytest.mark.parametrize("db", [0, 2, 4])
@pytest.mark.parametrize("method", [0, 1, 2, 3])
@pytest.mark.parametrize("iters", [5, 50])
def test_default_h_fixtures_f64(dec_by_schedule, golden, db, method, iters, prec, sched):
    """Every f64 mode, both kernel schedules (one wave per frame / one
    workgroup per frame) against the oracle's fixtures: modes 0 / 2 bit for
    bit including the posteriors, mode 3 (F64_FAST) decisions identical on
    these fixtures and posteriors within its stated tolerance."""
    dec = dec_by_schedule[sched]
    fd = golden("frames_default.npz")
    assert (dec.H == fd["H_reordered"]).all()
    llr = fd["db%d_llr" % db]
    out = dec.decode(llr, method=method, max_iters=iters, precision=prec, want_llr=True)
    key = "db%d_m%d_i%d" % (db, method, iters)
    np.testing.assert_array_equal(out["bits"], fd[key + "_bits"])
    np.testing.assert_array_equal(out["packed"], fd[key + "_packed"])
    np.testing.assert_array_equal(out["iters"], fd[key + "_iters"])
    np.testing.assert_array_equal(out["synd"], fd[key + "_synd"])
    if method == 0 or method >= 2 or prec in (0, 2):
        # exact in f64 (sum-product: glibc's tanh/log reproduced, ldpc_exact.hpp)
        np.testing.assert_array_equal(out["llr"], fd[key + "_post"])
    else:
        np.testing.assert_allclose(out["llr"], fd[key + "_post"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("db", [0, 2, 4])
@pytest.mark.parametrize("method", [0, 1])
def test_default_h_f32_hard_decisions(dec, golden, db, method):
    """f32: sum-product (ROCm's tanhf / logf: no host oracle, see
    tests/test_gpu_sumproduct_inexact.py for the assembled one) gives the f64
    oracle's hard decisions on these fixtures and posterior LLRs within the
    stated f32 tolerance; min-sum is the reference's arithmetic in float and
    equals the float oracle on every frame, posteriors bit for bit."""
    fd = golden("frames_default.npz")
    key = "db%d_m%d_i50" % (db, method)
    out = dec.decode(fd["db%d_llr" % db], method=method, max_iters=50, precision=1,
                     want_llr=True)
    mism = int((out["bits"] != fd[key + "_bits"]).any(axis=1).sum())
    if method == 1:
        assert mism == 0
        same = (out["iters"] == fd[key + "_iters"])
        ok = np.abs(out["llr"] - fd[key + "_post"]) <= 1e-3 * (1 + np.abs(fd[key + "_post"]))
        assert ok[same].all()
    else:
        # the float arithmetic parts from the double on frames that do not converge
        # quickly (75/2000 at 2 dB), so the f64 fixtures are no reference for
        # it; the float oracle is, on all frames
        from oracle import oracle as orc
        ref = orc.decode_batch(0, fd["H_reordered"], fd["db%d_llr" % db], 50, want_post=True,
                               real="f32")
        for k in ("bits", "packed", "iters", "synd"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
        np.testing.assert_array_equal(out["llr"].view(np.uint32), ref["post"].view(np.uint32))
        easy = fd[key + "_iters"] <= 5
        assert (out["bits"][easy] == fd[key + "_bits"][easy]).all()


@pytest.mark.parametrize("name", ["hData1", "hData2", "hData3", "hData5"])
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_other_h_matrices(golden, name, method):
    import ldpc_ece535a as L
    fo = golden("frames_other.npz")
    d = L.Decoder(golden("reference_data.npz")[name])
    assert (d.H == fo[name + "_H_reordered"]).all()
    out = d.decode(fo[name + "_llr"], method=method, max_iters=20, precision=0)
    np.testing.assert_array_equal(out["bits"], fo["%s_m%d_bits" % (name, method)])
    np.testing.assert_array_equal(out["iters"], fo["%s_m%d_iters" % (name, method)])
    np.testing.assert_array_equal(out["synd"], fo["%s_m%d_synd" % (name, method)])


def test_strided_complex_and_polarity(dec, golden):
    """Frames read from an interleaved gr_complex stream at any start
    offset, with tx = Re * polarity (general_work :149-153, :180-187)."""
    from oracle import oracle as orc
    fd = golden("frames_default.npz")
    y = fd["db2_llr"][:40].reshape(-1)
    z = np.zeros(2 * y.size + 10, np.float32)
    z[10::2] = y  # re parts after a 5-sample offset
    for pol in (1.0, -1.0):
        for stride in (128, 2):  # frame-aligned windows, then 1-sample steps
            B = 30
            out = dec.decode(z[10:], method=1, max_iters=50, polarity=pol, cw_stride=stride,
                             elem_stride=2, B=B)
            ref = orc.decode_batch(1, fd["H_reordered"], z[10:], 50, polarity=pol,
                                   cw_stride=stride, elem_stride=2, B=B)
            assert (out["bits"] == ref["bits"]).all() and (out["iters"] == ref["iters"]).all()


@pytest.mark.parametrize("B", [1, 3, 4, 5, 1023, 4097])
def test_batch_sizes(dec, golden, B):
    from oracle import oracle as orc
    rng = np.random.default_rng(B)
    y = (rng.standard_normal((B, 64)) + np.where(rng.random((B, 64)) < .5, 1, -1)).astype(
        np.float32)
    out = dec.decode(y, method=0, max_iters=20)
    ref = orc.decode_batch(0, dec.H, y, 20, nthreads=8)
    assert (out["bits"] == ref["bits"]).all() and (out["iters"] == ref["iters"]).all()
    assert (out["synd"] == ref["synd"]).all() and (out["packed"] == ref["packed"]).all()


def test_empty_batch(dec):
    out = dec.decode(np.zeros((0, 64), np.float32), method=1)
    assert out["packed"].shape == (0, 4)


def test_et_period(dec, golden):
    """et_period=5: checks only every 5th iteration -> iterations used are
    multiples of 5 (or the cap); converged frames still satisfy H c = 0."""
    fd = golden("frames_default.npz")
    out = dec.decode(fd["db4_llr"], method=1, max_iters=50, et_period=5)
    it = out["iters"]
    assert ((it % 5 == 0) | (it == 50)).all()
    ok = out["synd"] == 0
    assert ok.mean() > 0.8


def test_large_batch_noiseless_roundtrip(dec):
    """Size-independent property at full bench size: noiseless codewords of
    random data decode to their data bits, with 1 iteration, every method."""
    import ldpc_ece535a as L
    rng = np.random.default_rng(7)
    B = 65536
    data = rng.integers(0, 2, size=(B, 32), dtype=np.uint8)
    x = (2.0 * L.encode(dec.H, data) - 1.0).astype(np.float32)
    for method in (0, 1, 2, 3):
        out = dec.decode(x, method=method, max_iters=50)
        assert (out["packed"] == np.packbits(data, axis=1)).all()
        assert (out["synd"] == 0).all()
        assert (out["iters"] <= 1).all()


def test_unsupported_code_shape():
    import ldpc_ece535a as L
    H = np.zeros((300, 600), np.uint8)
    H[np.arange(300), np.arange(300)] = 1
    H[:, 300] = 1  # column degree 300
    with pytest.raises(L.LdpcError, match="outside the large-code kernels"):
        L.Decoder(H)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_non_finite_samples(golden, method, prec, graph):
    """Frames holding +-inf / NaN samples follow the reference's double
    arithmetic (inf messages, NaN propagation, sign(NaN) = 0) exactly; the
    sum-product kernel routes such frames to its select-based variant."""
    import ldpc_ece535a as L
    from oracle import oracle as orc
    fd = golden("frames_default.npz")
    y = fd["db2_llr"].copy()
    rng = np.random.default_rng(99)
    for b in range(0, y.shape[0], 3):  # every third frame gets 1-3 bad samples
        for _ in range(1 + b % 3):
            y[b, rng.integers(0, 64)] = rng.choice([np.inf, -np.inf, np.nan])
    d = L.Decoder(force_graph=graph)
    out = d.decode(y, method=method, max_iters=20, precision=prec)
    ref = orc.decode_batch(method, fd["H_reordered"], y, 20)
    np.testing.assert_array_equal(out["bits"], ref["bits"])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    np.testing.assert_array_equal(out["synd"], ref["synd"])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("method", [0, 1])
def test_extreme_finite_samples(golden, method, prec, graph):
    """Finite samples far outside the channel's range: amplitudes up to 1e30
    (tanh saturates to +-1, so T = +-1 gives +-inf check messages and inf - inf
    = NaN bit messages inside frames whose samples are all finite -- the
    select-free sum-product variant), and tiny / subnormal amplitudes.  The
    decoder must follow the reference's double arithmetic through all of it."""
    import ldpc_ece535a as L
    from oracle import oracle as orc
    fd = golden("frames_default.npz")
    base = fd["db2_llr"].astype(np.float64)
    parts = [base[:48] * a for a in (8.0, 30.0, 1e3, 1e10, 1e30, 1e-30, 1e-40)]
    y = np.concatenate(parts).astype(np.float32)
    assert np.isfinite(y).all()
    d = L.Decoder(force_graph=graph)
    out = d.decode(y, method=method, max_iters=30, precision=prec)
    ref = orc.decode_batch(method, fd["H_reordered"], y, 30)
    np.testing.assert_array_equal(out["bits"], ref["bits"])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    np.testing.assert_array_equal(out["synd"], ref["synd"])
