"""GPU parity of the on-chip decode path (ldpc_onchip.hip, LDPC_FLAG_ONCHIP):
one frame per workgroup, every message in LDS.

Every comparison is against the oracle (the golden fixtures it produced, its
sparse restatement for the mid-size codes, its dense form for posteriors),
never against the kernel itself: the reference's own matrices forced onto the
path, the N = 720 and N = 2160 IRA codes (several edges per thread), a code
at the kernels' degree limits, the frame queue at batches below and above the
resident workgroups, every input form of the C ABI, and the methods and
entry points the path hands on or refuses."""
import numpy as np
import pytest

from shape_cases import degree_limit_code as _degree_limit_code, same_bits as _same_bits

pytestmark = pytest.mark.gpu

KEYS = ("bits", "packed", "iters", "synd")


def _eq(out, ref, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))


def _code(K, N, hi_groups):
    from ldpc_ece535a import codes
    t = codes.dvbs2_like_table(3, K=K, N=N, hi_groups=hi_groups, hi_deg=6, lo_deg=3)
    return codes.ira_from_table(t, K, N)


def _noisy(csr, B, db, seed):
    from ldpc_ece535a import codes
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, csr[1] - csr[0]), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


def _dense(csr):
    M, N, rp, ci = csr
    H = np.zeros((M, N), np.uint8)
    H[np.repeat(np.arange(M), np.diff(rp)), ci] = 1
    return H


def _sparse_ref(csr, method, y, iters, **kw):
    from oracle import oracle as orc
    M, N, rp, ci = csr
    return orc.decode_batch_sparse(method, rp, ci, M, N, y, iters, nthreads=16, **kw)


def _early_and_capped(iters, cap):
    return (iters < cap).any() and (iters == cap).any()


class _Case:
    """A code, its on-chip decoder and oracle results computed once."""

    def __init__(self, csr):
        import ldpc_ece535a as L
        self.csr = csr
        self.dec = L.Decoder(csr=csr, onchip=True)
        assert self.dec.path == L._capi.PATH_ONCHIP == 2
        assert self.dec.pipeline() == {"frames_per_chunk": 0, "chunks": 0}
        with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED"):
            self.dec.layout_model
        self._refs = {}

    def ref(self, name, fn):
        if name not in self._refs:
            self._refs[name] = fn()
        return self._refs[name]


@pytest.fixture(scope="module")
def c720():
    c = _Case(_code(360, 720, 1))
    assert c.dec.E == 2879
    return c


@pytest.fixture(scope="module")
def c2160():
    c = _Case(_code(1080, 2160, 2))
    assert c.dec.E == 7559
    return c


# ---- 1. the reference's matrices through the new kernel ---------------------

@pytest.fixture(scope="module")
def odec():
    import ldpc_ece535a as L
    d = L.Decoder(onchip=True)
    assert d.path == L._capi.PATH_ONCHIP
    return d


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("db", [0, 2, 4])
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("iters", [5, 50])
def test_default_h_fixtures(odec, golden, db, method, iters, prec):
    fd = golden("frames_default.npz")
    assert (odec.H == fd["H_reordered"]).all()
    out = odec.decode(fd["db%d_llr" % db], method=method, max_iters=iters, precision=prec,
                      want_llr=True)
    key = "db%d_m%d_i%d" % (db, method, iters)
    _eq(out, {k: fd[key + "_" + k] for k in KEYS})
    _same_bits(out["llr"], fd[key + "_post"])


@pytest.mark.parametrize("name", ["hData1", "hData2", "hData3", "hData5"])
@pytest.mark.parametrize("method", [0, 1])
def test_other_h_fixtures(golden, name, method):
    import ldpc_ece535a as L
    fo = golden("frames_other.npz")
    d = L.Decoder(golden("reference_data.npz")[name], onchip=True)
    assert d.path == L._capi.PATH_ONCHIP
    out = d.decode(fo[name + "_llr"], method=method, max_iters=20, precision=0)
    for k in ("bits", "iters", "synd"):
        np.testing.assert_array_equal(out[k], fo["%s_m%d_%s" % (name, method, k)], err_msg=k)


# ---- 2. N = 720 against the sparse and dense oracles --------------------------

def _frames720(c):
    def make():
        y = _noisy(c.csr, 256, 3.0, 5)
        # the special samples of test_non_finite, on a stride of frames
        y[::7, 3] = np.inf
        y[1::5, 10] = -np.inf
        y[2::9, 20] = np.nan
        y[3::4, 30:34] = 0.0
        y[5::8, 400:404] = -0.0
        return y
    return c.ref("y720", make)


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("method", [0, 1])
def test_n720_vs_oracle(c720, method, prec):
    from oracle import oracle as orc
    y = _frames720(c720)
    ref = c720.ref(("sparse", method), lambda: _sparse_ref(c720.csr, method, y, 30))
    assert _early_and_capped(ref["iters"], 30), (ref["iters"].min(), ref["iters"].max())
    post = c720.ref(("dense", method), lambda: orc.decode_batch(
        method, _dense(c720.csr), y[:64], 30, nthreads=16, want_post=True))
    _eq(post, {k: ref[k][:64] for k in KEYS}, what="dense vs sparse oracle")
    out = c720.dec.decode(y, method=method, max_iters=30, precision=prec, want_llr=True)
    _eq(out, ref)
    _same_bits(out["llr"][:64], post["post"])


# ---- 3. N = 2160: several edges per thread ------------------------------------

@pytest.mark.parametrize("method,db", [(0, 2.0), (1, 3.0)])
def test_n2160_vs_oracle(c2160, method, db):
    """48 frames at the Eb/N0 where the method's frames both stop early and
    reach the cap of 20 (the oracle's iterations, seed 6: min-sum 7..20 at
    2 dB, sum-product 10..20 at 3 dB)."""
    from oracle import oracle as orc
    y = _noisy(c2160.csr, 48, db, 6)
    ref = _sparse_ref(c2160.csr, method, y, 20)
    assert _early_and_capped(ref["iters"], 20), (ref["iters"].min(), ref["iters"].max())
    post = orc.decode_batch(method, _dense(c2160.csr), y[:8], 20, nthreads=8, want_post=True)
    out = c2160.dec.decode(y, method=method, max_iters=20, precision=0, want_llr=True)
    _eq(out, ref)
    _same_bits(out["llr"][:8], post["post"])


# ---- 4. the kernels' degree limits ---------------------------------------------

@pytest.mark.parametrize("method", [0, 1])
def test_degree_limits(method):
    import ldpc_ece535a as L
    csr, H = _degree_limit_code()
    dc, dv = H.sum(axis=1), H.sum(axis=0)
    assert dc.max() == 32 and dc.min() == 1 and dv.max() == 16 and dv.min() == 1
    d = L.Decoder(csr=csr, onchip=True)
    assert d.path == L._capi.PATH_ONCHIP and (d.dc_max, d.dv_max) == (32, 16)
    rng = np.random.Generator(np.random.PCG64(41))
    y = (-1.0 + np.sqrt(10 ** (-5.0 / 10)) * rng.standard_normal((512, 120))).astype(np.float32)
    ref = _sparse_ref(csr, method, y, 20)
    if method == 0:
        assert _early_and_capped(ref["iters"], 20), (ref["iters"].min(), ref["iters"].max())
    out = d.decode(y, method=method, max_iters=20, precision=0)
    _eq(out, ref)


# ---- 5. queue and batch shapes ---------------------------------------------------

def _queue_frames(c):
    return c.ref("yq", lambda: _noisy(c.csr, 5000, 4.0, 8))


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(c720, method, B):
    y = _queue_frames(c720)[:B]
    _eq(c720.dec.decode(y, method=method, max_iters=8), _sparse_ref(c720.csr, method, y, 8))


@pytest.mark.parametrize("cap,method", [(8, 0), (12, 1)], ids=["stride", "counter"])
def test_more_frames_than_workgroups(c720, cap, method):
    """5000 frames on far fewer resident workgroups: at cap 8 each workgroup
    walks the batch at a fixed stride (DecodeArgs::static_stride, caps <= 10),
    at cap 12 it pulls frames from the stream's counter.  The same batch then
    runs on a second stream of the same context (its own counter), on the
    first again, whose counter has advanced by the first launch, and on the
    second again."""
    import torch
    y = _queue_frames(c720)
    ref = _sparse_ref(c720.csr, method, y, cap)
    dec = c720.dec
    _eq(dec.decode(y, method=method, max_iters=cap), ref)
    d_y = torch.from_numpy(y).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (side.cuda_stream, None, side.cuda_stream):
        pk = torch.zeros((5000, dec.KB), dtype=torch.uint8, device="cuda")
        it = torch.full((5000,), -1, dtype=torch.int32, device="cuda")
        sy = torch.full((5000,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_device(d_y.data_ptr(), 5000, pk.data_ptr(), method=method, max_iters=cap,
                          d_iters=it.data_ptr(), d_synd=sy.data_ptr(), stream=stream)
        side.synchronize()
        dec.synchronize()
        _eq(dict(packed=pk.cpu().numpy(), iters=it.cpu().numpy(), synd=sy.cpu().numpy()), ref,
            keys=("packed", "iters", "synd"), what="stream %r" % (stream,))


@pytest.mark.parametrize("method", [0, 1])
def test_et_period_and_single_iteration(c720, method):
    y = _queue_frames(c720)[:300]
    out = c720.dec.decode(y, method=method, max_iters=50, et_period=5)
    ref = _sparse_ref(c720.csr, method, y, 50, et_period=5)
    assert (ref["iters"] % 5 == 0).all()
    _eq(out, ref, what="et_period 5")
    _eq(c720.dec.decode(y, method=method, max_iters=1), _sparse_ref(c720.csr, method, y, 1),
        what="one iteration")


# ---- 6. input forms ----------------------------------------------------------------

def _complex_stream(c):
    def make():
        y = _noisy(c.csr, 6, 4.0, 9).reshape(-1)
        z = np.zeros(2 * y.size + 10, np.float32)
        z[10::2] = y
        z[11::2] = np.random.Generator(np.random.PCG64(10)).standard_normal(y.size)
        return z
    return c.ref("z", make)


@pytest.mark.parametrize("pol", [1.0, -1.0])
def test_strided_complex_polarity(c720, pol):
    """Interleaved gr_complex samples, windows sliding by one sample
    (cw_stride = elem_stride = 2), either polarity."""
    from oracle import oracle as orc
    z = _complex_stream(c720)
    M, N, rp, ci = c720.csr
    B = min(150, (z.size - 10 - 2 * N) // 2)
    out = c720.dec.decode(z[10:], method=1, max_iters=10, polarity=pol, cw_stride=2,
                          elem_stride=2, B=B)
    ref = orc.decode_batch_sparse(1, rp, ci, M, N, z[10:], 10, polarity=pol, cw_stride=2,
                                  elem_stride=2, B=B, nthreads=16)
    _eq(out, ref)


@pytest.mark.parametrize("method", [0, 1])
def test_decode_both_polarities(c720, method):
    from oracle import oracle as orc
    z = _complex_stream(c720)
    M, N, rp, ci = c720.csr
    B = 40
    both = c720.dec.decode_both(z[10:], method=method, max_iters=12, cw_stride=2 * N // 8,
                                elem_stride=2, B=B)
    for half, pol in ((0, 1.0), (1, -1.0)):
        ref = orc.decode_batch_sparse(method, rp, ci, M, N, z[10:], 12, polarity=pol,
                                      cw_stride=2 * N // 8, elem_stride=2, B=B, nthreads=16)
        _eq({k: both[k][half * B:(half + 1) * B] for k in ("packed", "synd")}, ref,
            keys=("packed", "synd"), what="polarity %g" % pol)


@pytest.mark.parametrize("method", [0, 1])
def test_decode_windows_mixed_signs(c720, method):
    z = _complex_stream(c720)[10:]
    span = z[0::2]
    N = c720.dec.N
    rng = np.random.default_rng(9)
    pos = np.concatenate([N * np.arange(3), rng.integers(0, span.size - N, 37)])
    neg = rng.integers(0, 2, pos.size)
    win = (pos.astype(np.int64) << 1) | neg
    out = c720.dec.decode_windows(z, win, method=method, max_iters=12, elem_stride=2)
    frames = np.stack([span[p:p + N] for p in pos])
    for sign in (0, 1):
        ref = _sparse_ref(c720.csr, method, frames[neg == sign], 12,
                          polarity=-1.0 if sign else 1.0)
        _eq({k: out[k][neg == sign] for k in ("packed", "synd")}, ref, keys=("packed", "synd"),
            what="negate %d" % sign)
    again = c720.dec.decode_windows(z, win[::-1].copy(), method=method, max_iters=12,
                                    elem_stride=2, reuse_span=True)
    _eq({k: again[k][::-1] for k in ("packed", "synd")}, out, keys=("packed", "synd"))


# ---- 7. the other methods, and what the path refuses ------------------------------

@pytest.mark.parametrize("method", [2, 3])
def test_bitflip_and_hard_on_onchip_context(c720, method):
    y = _queue_frames(c720)[:200]
    _eq(c720.dec.decode(y, method=method, max_iters=10), _sparse_ref(c720.csr, method, y, 10))


def test_ring_and_server_are_refused(c720):
    import ldpc_ece535a as L
    y = _queue_frames(c720)[:16]
    ref = _sparse_ref(c720.csr, 1, y, 8)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*on-chip"):
        c720.dec.ring_begin(method=1, max_iters=8)
    _eq(c720.dec.decode(y, method=1, max_iters=8), ref, what="after ring_begin")
    c720.dec.stage_span(y.reshape(-1), max_windows=16)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*on-chip"):
        c720.dec.serve_begin(method=1, max_iters=8, max_windows=16)
    _eq(c720.dec.decode(y, method=1, max_iters=8), ref, what="after serve_begin")


# ---- 8. the inexact modes ------------------------------------------------------------

@pytest.mark.parametrize("prec", [1, 3])
@pytest.mark.parametrize("method", [0, 1])
def test_inexact_modes_equal_large_code_path(odec, golden, method, prec):
    """Sum-product at precisions 1 (f32) and 3 (compact f64) has no host
    oracle (tests/test_gpu_sumproduct_inexact.py holds both paths to one
    assembled from the device's functions);
    the large-code kernels evaluate the same scalar Math<PREC> calls in the
    same order with contraction off, so every output is equal, posteriors bit
    for bit.  Min-sum has one at either precision: the oracle's float
    restatement at f32, the oracle itself (its fixtures) at the compact f64
    mode, which for min-sum is plain double arithmetic."""
    import ldpc_ece535a as L
    from oracle import oracle as orc
    fd = golden("frames_default.npz")
    g = L.Decoder(force_graph=True)
    for db in (0, 2, 4):
        for iters in (5, 50):
            what = "db %d iters %d" % (db, iters)
            kw = dict(method=method, max_iters=iters, precision=prec, want_llr=True)
            a = odec.decode(fd["db%d_llr" % db], **kw)
            b = g.decode(fd["db%d_llr" % db], **kw)
            _eq(a, b, what=what)
            _same_bits(a["llr"], b["llr"], what=what)
            if method == 0:
                if prec == 1:
                    ref = orc.decode_batch(0, fd["H_reordered"], fd["db%d_llr" % db], iters,
                                           want_post=True, real="f32")
                else:
                    key = "db%d_m0_i%d_" % (db, iters)
                    ref = {k: fd[key + k] for k in KEYS + ("post",)}
                _eq(a, ref, what=what + ", on-chip vs oracle")
                _same_bits(a["llr"], ref["post"], what=what + ", on-chip vs oracle")
