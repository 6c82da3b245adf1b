"""GPU parity of the layered normalized min-sum decoder (ldpc_layered.hip,
ldpc_decode_layered*): one frame per workgroup, posteriors and check messages
in LDS, the rows of H taken layer by layer.

Every comparison is against the numpy restatement of the contract
(tests/layered_ref.py, pinned on the CPU by tests/test_layered_host.py) run
with the plan the decoder reports, never against the kernel itself: bits,
packed bytes, iteration counts, syndrome weights, and the posteriors as bit
patterns."""
import numpy as np
import pytest

import layered_ref as lref
from shape_cases import degree_limit_code, same_bits

pytestmark = pytest.mark.gpu

KEYS = lref.KEYS


def _eq(out, ref, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))
    if "llr" in out:
        same_bits(out["llr"], ref["llr"], what=what)


def _early_and_capped(iters, cap):
    return (iters < cap).any() and (iters == cap).any()


class _Case:
    """A code, a decoder for it and restatement results computed once."""

    def __init__(self, csr, **kw):
        import ldpc_ece535a as L
        self.csr = csr
        self.dec = L.Decoder(csr=csr, **kw)
        self.plan = self.dec.layers
        assert (self.plan == L.plan_layers(csr)["layer_of_row"]).all()
        self._refs = {}

    def memo(self, name, fn):
        if name not in self._refs:
            self._refs[name] = fn()
        return self._refs[name]

    def ref(self, name, y, cap, plan=None, **kw):
        return self.memo((name, cap, tuple(sorted(kw.items()))), lambda: lref.decode(
            self.csr, self.plan if plan is None else plan, y, cap, **kw))


@pytest.fixture(scope="module")
def c720():
    c = _Case(lref.ira_code(360, 720, 1), onchip=True)
    assert c.dec.E == 2879 and int(c.plan.max()) + 1 == 14
    return c


# ---- 1. the reference's default H on every kind of context -------------------------

_default_refs = {}


@pytest.fixture(scope="module")
def default_decs():
    import ldpc_ece535a as L
    decs = {"default": L.Decoder(), "graph": L.Decoder(force_graph=True),
            "onchip": L.Decoder(onchip=True)}
    assert [d.path for d in decs.values()] == [0, 1, 2]
    return decs


@pytest.mark.parametrize("scale", [1.0, 0.8125])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cap", [5, 50])
@pytest.mark.parametrize("kind", ["default", "graph", "onchip"])
def test_default_h(default_decs, golden, kind, cap, prec, scale):
    fd = golden("frames_default.npz")
    dec = default_decs[kind]
    assert (dec.H == fd["H_reordered"]).all()
    csr = (dec.M, dec.N, dec.row_ptr, dec.col_idx)
    plan = dec.layers
    assert int(plan.max()) + 1 == 7
    for db in (0, 2, 4):
        y = fd["db%d_llr" % db]
        key = (db, cap, prec, scale)
        if key not in _default_refs:
            _default_refs[key] = lref.decode(csr, plan, y, cap, scale=scale, precision=prec)
        out = dec.decode_layered(y, scale=scale, max_iters=cap, precision=prec, want_llr=True)
        _eq(out, _default_refs[key], what="db %d" % db)


# ---- 2. N = 720: special samples, early and capped frames ---------------------------

def _frames720(c):
    def make():
        y = lref.noisy(c.csr, 256, 2.0, 5)
        # the special samples of tests/test_gpu_onchip.py, on a stride of frames
        y[::7, 3] = np.inf
        y[1::5, 10] = -np.inf
        y[2::9, 20] = np.nan
        y[3::4, 30:34] = 0.0
        y[5::8, 400:404] = -0.0
        return y
    return c.memo("y720", make)


@pytest.mark.parametrize("scale", [1.0, 0.8125])
def test_n720(c720, scale):
    y = _frames720(c720)
    ref = c720.ref("y720", y, 30, scale=scale)
    assert _early_and_capped(ref["iters"], 30), (ref["iters"].min(), ref["iters"].max())
    _eq(c720.dec.decode_layered(y, scale=scale, max_iters=30, want_llr=True), ref)


# ---- 3. larger codes: several rows per thread's layer, tables in L2 -----------------

def test_n2160():
    """Layers of up to 192 rows on a three-wave workgroup; 48 frames at 2 dB
    (seed 6), where the restatement's iterations run 4..20 at cap 20."""
    import ldpc_ece535a as L
    c = _Case(lref.ira_code(1080, 2160, 2), onchip=True)
    assert c.dec.E == 7559
    assert L.plan_layers(c.csr)["threads"] == 192
    y = lref.noisy(c.csr, 48, 2.0, 6)
    ref = c.ref("y", y, 20)
    assert _early_and_capped(ref["iters"], 20), (ref["iters"].min(), ref["iters"].max())
    _eq(c.dec.decode_layered(y, max_iters=20, want_llr=True), ref)


@pytest.mark.parametrize("prec", [0, 1])
def test_n4320_at_the_lds_limit(prec):
    """E = 15119: in double a frame's state is 159968 of the 163840 bytes and
    the tables stay in L2; in float they are staged behind it.  Layers wider
    than one wave (320 threads)."""
    import ldpc_ece535a as L
    csr = lref.ira_code(2160, 4320, 4)
    p = L.plan_layers(csr, precision=prec)
    frame = (4 if prec else 8) * (4320 + 15119) + 4320 + 128
    assert p["fits"] and p["threads"] == 320
    if prec == 0:    # the frame alone, each array padded to 16 bytes
        assert frame <= p["lds_bytes"] == 159968 < frame + 64
    else:            # rows, 16-bit columns and row order behind the frame
        assert p["lds_bytes"] > frame + 4 * 2160 + 2 * 15119 + 2 * 2160
    c = _Case(csr)                       # a plain large-code context
    assert c.dec.path == 1
    y = lref.noisy(csr, 20, 1.8, 12)     # the restatement's iterations run 5..10 at cap 10
    ref = c.ref("y", y, 10, precision=prec)
    assert _early_and_capped(ref["iters"], 10), (ref["iters"].min(), ref["iters"].max())
    _eq(c.dec.decode_layered(y, max_iters=10, precision=prec, want_llr=True), ref)


# ---- 4. degree limits ------------------------------------------------------------------

@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.8125])
def test_degree_limits(scale, prec):
    """A row of degree 32, one-row layers, a row and a column of degree 1."""
    csr, H = degree_limit_code()
    dc, dv = H.sum(axis=1), H.sum(axis=0)
    assert dc.max() == 32 and dc.min() == 1 and dv.max() == 16 and dv.min() == 1
    c = _Case(csr, onchip=True)
    assert int(c.plan.max()) + 1 == 16 and (np.bincount(c.plan) == 1).any()
    rng = np.random.Generator(np.random.PCG64(41))
    y = (-1.0 + np.sqrt(10 ** (-5.0 / 10)) * rng.standard_normal((512, 120))).astype(np.float32)
    ref = c.ref("y", y, 20, scale=scale, precision=prec)
    assert _early_and_capped(ref["iters"], 20), (ref["iters"].min(), ref["iters"].max())
    _eq(c.dec.decode_layered(y, scale=scale, max_iters=20, precision=prec, want_llr=True), ref)


# ---- 5. plans -----------------------------------------------------------------------------

def test_set_layers(c720):
    import ldpc_ece535a as L
    dec, M = c720.dec, c720.dec.M
    y = _frames720(c720)[:64]
    planned = lref.decode(c720.csr, c720.plan, y, 30)
    _eq(dec.decode_layered(y, max_iters=30, want_llr=True), planned, what="planner's plan")
    try:
        serial = np.arange(M, dtype=np.int32)     # one row per layer, natural order
        dec.set_layers(serial)
        assert (dec.layers == serial).all()
        ref = lref.decode(c720.csr, serial, y, 30)
        out = dec.decode_layered(y, max_iters=30, want_llr=True)
        _eq(out, ref, what="one row per layer")
        assert (out["iters"] != planned["iters"]).any() or (
            out["llr"].view(np.uint32) != planned["llr"].view(np.uint32)).any()
        # rows 0 and 1 of the staircase share column 0
        rp, ci = c720.csr[2], c720.csr[3]
        shared = np.intersect1d(ci[rp[0]:rp[1]], ci[rp[1]:rp[2]])
        assert shared.size
        bad = serial.copy()
        bad[1] = 0
        with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*rows 0 and 1 .*column %d" % shared[0]):
            dec.set_layers(bad)
        bad = serial.copy()
        bad[5] = M
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*row 5"):
            dec.set_layers(bad)
        assert (dec.layers == serial).all()
        _eq(dec.decode_layered(y, max_iters=30, want_llr=True), ref, what="after refused plans")
    finally:
        dec.set_layers(None)
    assert (dec.layers == c720.plan).all()
    _eq(dec.decode_layered(y, max_iters=30, want_llr=True), planned, what="planner's plan restored")


# ---- 6. the frame queue ---------------------------------------------------------------------

def _queue_frames(c):
    return c.memo("yq", lambda: lref.noisy(c.csr, 5000, 4.0, 8))


@pytest.mark.parametrize("cap,scale", [(8, 1.0), (12, 0.8125)], ids=["stride", "counter"])
def test_more_frames_than_workgroups(c720, cap, scale):
    """5000 frames on far fewer resident workgroups: a fixed stride at cap 8,
    the stream's counter at cap 12; then on a second stream of the same
    context, on the first again and on the second again."""
    import torch
    y = _queue_frames(c720)
    ref = c720.ref("yq", y, cap, scale=scale)
    dec = c720.dec
    _eq(dec.decode_layered(y, scale=scale, max_iters=cap, want_llr=True), ref)
    d_y = torch.from_numpy(y).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (side.cuda_stream, None, side.cuda_stream):
        pk = torch.zeros((5000, dec.KB), dtype=torch.uint8, device="cuda")
        bt = torch.zeros((5000, dec.N), dtype=torch.uint8, device="cuda")
        it = torch.full((5000,), -1, dtype=torch.int32, device="cuda")
        sy = torch.full((5000,), -1, dtype=torch.int32, device="cuda")
        po = torch.zeros((5000, dec.N), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_layered_device(d_y.data_ptr(), 5000, pk.data_ptr(), scale=scale, max_iters=cap,
                                  d_bits=bt.data_ptr(), d_iters=it.data_ptr(),
                                  d_synd=sy.data_ptr(), d_llr=po.data_ptr(), stream=stream)
        side.synchronize()
        dec.synchronize()
        _eq(dict(packed=pk.cpu().numpy(), bits=bt.cpu().numpy(), iters=it.cpu().numpy(),
                 synd=sy.cpu().numpy(), llr=po.cpu().numpy()), ref, what="stream %r" % (stream,))


# ---- 7. exit rule and batch shapes ------------------------------------------------------------

def test_et_period_and_single_iteration(c720):
    y = np.concatenate([_queue_frames(c720)[:100], _frames720(c720)[:24]])
    ref = lref.decode(c720.csr, c720.plan, y, 50, et_period=5)
    assert (ref["iters"] % 5 == 0).all() and _early_and_capped(ref["iters"], 50)
    _eq(c720.dec.decode_layered(y, max_iters=50, et_period=5, want_llr=True), ref,
        what="et_period 5")
    _eq(c720.dec.decode_layered(y, max_iters=1, want_llr=True),
        lref.decode(c720.csr, c720.plan, y, 1), what="one iteration")


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(c720, B):
    y = _frames720(c720)[:B]
    _eq(c720.dec.decode_layered(y, scale=0.8125, max_iters=12, want_llr=True),
        lref.decode(c720.csr, c720.plan, y, 12, scale=0.8125))


# ---- 8. input forms ------------------------------------------------------------------------------

def test_strided_complex_negative_polarity(c720):
    """Interleaved gr_complex samples, windows sliding by one sample
    (cw_stride = elem_stride = 2) at polarity -1, through the host entry
    point; the frames hold -codeword + noise so that some decode."""
    N = c720.dec.N
    B = 40
    base = -lref.noisy(c720.csr, 2, 3.0, 9).reshape(-1)
    z = np.zeros(2 * base.size + 10, np.float32)
    z[10::2] = base
    z[11::2] = np.random.Generator(np.random.PCG64(10)).standard_normal(base.size)
    frames = np.stack([z[10::2][s:s + N] for s in range(B)])         # window 0 is a frame
    ref = lref.decode(c720.csr, c720.plan, frames, 10, scale=0.8125, polarity=-1.0)
    assert _early_and_capped(ref["iters"], 10)
    out = c720.dec.decode_layered(z[10:], scale=0.8125, max_iters=10, polarity=-1.0, cw_stride=2,
                                  elem_stride=2, B=B, want_llr=True)
    _eq(out, ref)
    # a contiguous real stream with a frame stride wider than N
    wide = np.zeros((B, N + 8), np.float32)
    wide[:, :N] = frames
    _eq(c720.dec.decode_layered(wide, scale=0.8125, max_iters=10, polarity=-1.0, cw_stride=N + 8,
                                want_llr=True), ref, what="cw_stride N + 8")


# ---- 9. refusals and neighbours -------------------------------------------------------------------

def test_bad_scale_is_refused(c720):
    import ldpc_ece535a as L
    y = _frames720(c720)[:4]
    for scale in (0.0, 1.5, float("nan"), -0.5, float("inf")):
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*scale"):
            c720.dec.decode_layered(y, scale=scale, max_iters=5)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL"):
        c720.dec.decode_layered(y, max_iters=0)


def test_code_beyond_the_lds_is_refused():
    import ldpc_ece535a as L
    from ldpc_ece535a import codes
    dec = L.Decoder(csr=codes.dvbs2_like(0))
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*bytes of LDS"):
        dec.decode_layered(np.zeros((1, dec.N), np.float32), max_iters=2)


def test_refused_while_a_ring_session_is_open(default_decs, golden):
    import ldpc_ece535a as L
    fd = golden("frames_default.npz")
    dec = default_decs["default"]
    y = fd["db2_llr"]
    csr = (dec.M, dec.N, dec.row_ptr, dec.col_idx)
    ref = lref.decode(csr, dec.layers, y, 50, scale=0.8125)
    dec.ring_begin(method=1, max_iters=50)
    try:
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*ring"):
            dec.decode_layered(y, scale=0.8125)
    finally:
        dec.ring_end()
    dec.synchronize()
    _eq(dec.decode_layered(y, scale=0.8125, want_llr=True), ref, what="after the ring session")
    out = dec.decode(y, method=0, max_iters=50)
    _eq(out, {k: fd["db2_m0_i50_" + k] for k in KEYS}, what="min-sum after layered decodes")


def test_ber_sweep_fifth_curve(default_decs):
    from ldpc_ece535a import ber
    dec = default_decs["default"]
    four = ber.sweep(dec, [2.0, 8.0], frames=30, iterations=5, seed=3)
    five = ber.sweep(dec, [2.0, 8.0], frames=30, iterations=5, seed=3, layered_scale=0.8125)
    assert list(five) == [n for n, _ in ber.METHODS] + [ber.LAYERED] and list(four) == list(five)[:4]
    assert all(five[n] == four[n] for n in four)
    lay = five[ber.LAYERED]
    assert len(lay["ber"]) == len(lay["fer"]) == 2 and all(0.0 <= v <= 1.0 for v in lay["ber"])
    assert all(0 <= v <= 30 for v in lay["fer"])
    assert "ber4=[" in ber.octave([2.0, 8.0], five) and "ber4" not in ber.octave([2.0, 8.0], four)


def test_min_sum_on_the_same_context_still_equals_the_oracle(c720):
    """Last in the file: after every layered decode above, the context's own
    min-sum route is what it was."""
    from oracle import oracle as orc
    M, N, rp, ci = c720.csr
    y = _queue_frames(c720)[:200]
    ref = orc.decode_batch_sparse(0, rp, ci, M, N, y, 12, nthreads=16)
    _eq(c720.dec.decode(y, method=0, max_iters=12), ref)
