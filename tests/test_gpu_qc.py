"""GPU parity of the layered decoder on quasi-cyclic contexts (ldpc_create_qc,
ldpc_layered.hip): the block rows as the plan, a thread per row of a block
row, columns from the base matrix.

Every comparison is against the numpy restatement of the layered contract
(tests/layered_ref.py) run on the expanded CSR with the block-row plan, never
against the kernel itself: bits, packed bytes, iteration counts, syndrome
weights, and the posteriors as bit patterns.  The codes are synthetic
(tests/qc_cases.py)."""
import numpy as np
import pytest

import layered_ref as lref
import qc_cases as qc
from shape_cases import same_bits

pytestmark = pytest.mark.gpu

KEYS = lref.KEYS


def _eq(out, ref, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))
    if "llr" in out:
        same_bits(out["llr"], ref["llr"], what=what)


def _early_and_capped(iters, cap):
    return (iters < cap).any() and (iters == cap).any()


def _differs(a, b):
    return (a["iters"] != b["iters"]).any() or (
        a["llr"].view(np.uint32) != b["llr"].view(np.uint32)).any()


class _Case:
    """A quasi-cyclic code, a decoder made from its base matrix, and
    restatement results computed once."""

    def __init__(self, name, base=None, Z=None, **kw):
        import ldpc_ece535a as L
        self.base, self.Z = qc.base_of(name) if base is None else (base, Z)
        self.mb = self.base.shape[0]
        self.csr = L.plan_qc(self.base, self.Z)["csr"]        # fails here without the feature
        self.dec = L.Decoder(qc=(self.base, self.Z), **kw)
        self.plan = qc.block_rows(self.mb, self.Z)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def frames(self, fseed, B, db):
        return self.memo(("y", fseed, B, db), lambda: qc.frames(self.csr, fseed, B, db))

    def ref(self, name, y, cap, plan=None, **kw):
        return self.memo((name, cap, plan is None, tuple(sorted(kw.items()))), lambda: lref.decode(
            self.csr, self.plan if plan is None else plan, y, cap, **kw))


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _frames_a(c):
    return c.memo("ya", lambda: qc.plant_special(c.frames(*qc.TABLE["A"][2][:3]).copy()))


# ---- 1. the cases of the table -----------------------------------------------------------

def _table_runs():
    runs = []
    for name in "ABCDEFG":
        precs = (0, 1) if name in "AG" else (qc.TABLE[name][2][4],)
        scales = (1.0, 0.8125) if name in "AG" else (1.0,)
        runs += [(name, p, s) for p in precs for s in scales]
    return runs


@pytest.mark.parametrize("name,prec,scale", _table_runs())
def test_cases(name, prec, scale):
    """A: Z = 64, special samples planted.  B: Z = 27, below a wave, the wrap
    inside it.  C: rows of 11..17 places on 1.5 waves.  D: six waves.  E: Z = 1.
    F: 1024 threads, float.  G: rows of 32, 23, 12 and 1 places."""
    c = case(name)
    if name == "G":
        fseed, B, db, cap = qc.G_FRAMES
        y = c.frames(fseed, B, db)
    else:
        assert (c.csr[1], c.csr[3].size) == qc.TABLE[name][1]
        fseed, B, db, cap = qc.TABLE[name][2][:4]
        y = _frames_a(c) if name == "A" else c.frames(fseed, B, db)
    assert c.dec.qc[1] == c.Z and (c.dec.qc[0] == c.base).all()
    assert (c.dec.row_ptr == c.csr[2]).all() and (c.dec.col_idx == c.csr[3]).all()
    ref = c.ref("table", y, cap, scale=scale, precision=prec)
    assert _early_and_capped(ref["iters"], cap), (ref["iters"].min(), ref["iters"].max())
    _eq(c.dec.decode_layered(y, scale=scale, max_iters=cap, precision=prec, want_llr=True), ref)


def test_empty_block_row():
    """A block row without a circulant (the kernel's table leaves it out) and
    a block column without one; noise around the all-zero codeword."""
    base = np.array([[0, -1, 3, -1, 5, 1],
                     [-1, -1, -1, -1, -1, -1],
                     [2, 0, -1, -1, 6, 4]], np.int32)
    c = _Case("empty", base, 7)
    assert (np.diff(c.csr[2]).reshape(3, 7) == np.array([4, 0, 4])[:, None]).all()
    rng = np.random.Generator(np.random.PCG64(112))
    y = (-1.0 + np.sqrt(10 ** (-1.0 / 10)) * rng.standard_normal((96, 42))).astype(np.float32)
    for scale in (1.0, 0.8125):
        ref = lref.decode(c.csr, c.plan, y, 10, scale=scale)
        assert _early_and_capped(ref["iters"], 10)
        _eq(c.dec.decode_layered(y, scale=scale, max_iters=10, want_llr=True), ref)
    c.dec.close()


# ---- 2. the default plan is the block rows ----------------------------------------------------

def test_fresh_context_decodes_by_block_rows():
    import ldpc_ece535a as L
    c = _Case("A")                                     # a context nothing has touched
    assert (c.dec.layers == np.repeat(np.arange(c.mb), c.Z)).all()
    first_fit = L.plan_layers(c.csr)["layer_of_row"]
    assert (first_fit != c.plan).any() and (first_fit == lref.first_fit(c.csr)).all()
    y = _frames_a(case("A"))
    out = c.dec.decode_layered(y, max_iters=20, want_llr=True)
    _eq(out, case("A").ref("table", y, 20, scale=1.0, precision=0))
    assert _differs(out, lref.decode(c.csr, first_fit, y, 20))
    plain = L.Decoder(csr=c.csr)                       # the same H, not quasi-cyclic
    assert plain.qc is None and (plain.layers == first_fit).all()
    plain.close()
    c.dec.close()


# ---- 3. other plans on a quasi-cyclic context -------------------------------------------------

def test_set_layers():
    import ldpc_ece535a as L
    c = case("A")
    y = _frames_a(c)
    rows = c.ref("table", y, 20, scale=1.0, precision=0)
    first_fit = L.plan_layers(c.csr)["layer_of_row"]
    try:
        c.dec.set_layers(first_fit)
        assert (c.dec.layers == first_fit).all()
        ref = lref.decode(c.csr, first_fit, y, 20)
        out = c.dec.decode_layered(y, max_iters=20, want_llr=True)
        _eq(out, ref, what="first fit (the table kernel)")
        assert _differs(out, rows)
        c.dec.set_layers(c.plan)                   # the block rows, set by the caller
        _eq(c.dec.decode_layered(y, max_iters=20, want_llr=True), rows, what="block rows set")
        c.dec.set_layers(first_fit)
        _eq(c.dec.decode_layered(y, max_iters=20, want_llr=True), ref, what="first fit again")
    finally:
        c.dec.set_layers(None)
    assert (c.dec.layers == c.plan).all()
    _eq(c.dec.decode_layered(y, max_iters=20, want_llr=True), rows, what="block rows restored")


# ---- 4. the table kernel under the same plan --------------------------------------------------

@pytest.mark.parametrize("name", ["B", "C"])
def test_table_kernel_cross_check(name):
    c = case(name)
    fseed, B, db, cap = qc.TABLE[name][2][:4]
    y = c.frames(fseed, B, db)
    ref = c.ref("table", y, cap, scale=1.0, precision=0)
    tab = _Case(name, qc_tables=True)
    assert (tab.dec.layers == c.plan).all()
    a = c.dec.decode_layered(y, max_iters=cap, want_llr=True)
    b = tab.dec.decode_layered(y, max_iters=cap, want_llr=True)
    _eq(a, ref, what="circulant kernel")
    _eq(b, ref, what="table kernel")
    _eq(a, b, what="circulant vs table kernel")
    tab.dec.close()


# ---- 5. the LDS boundary ----------------------------------------------------------------------

def test_lds_boundary():
    import ldpc_ece535a as L
    inside = _Case("inside", qc.boundary_base(39), 384)
    assert L.plan_qc(inside.base, 384)["lds_bytes"] == 161408
    y = inside.frames(109, 8, 3.0)
    _eq(inside.dec.decode_layered(y, max_iters=6, want_llr=True),
        lref.decode(inside.csr, inside.plan, y, 6), what="161408 bytes")
    inside.dec.close()
    beyond = _Case("beyond", qc.boundary_base(40), 384)
    assert not L.plan_qc(beyond.base, 384)["fits"] and L.plan_qc(beyond.base, 384, 1)["fits"]
    y = beyond.frames(110, 8, 3.0)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*bytes of LDS"):
        beyond.dec.decode_layered(y, max_iters=6)
    _eq(beyond.dec.decode_layered(y, max_iters=6, precision=1, want_llr=True),
        lref.decode(beyond.csr, beyond.plan, y, 6, precision=1), what="float")
    from oracle import oracle as orc
    M, N, rp, ci = beyond.csr
    _eq(beyond.dec.decode(y, method=0, max_iters=6),
        orc.decode_batch_sparse(0, rp, ci, M, N, y, 6, nthreads=16), what="min-sum")
    beyond.dec.close()


# ---- 6. the frame queue -----------------------------------------------------------------------

def _queue_frames(c):
    return c.frames(108, 5000, 4.0)


@pytest.mark.parametrize("cap,scale", [(8, 1.0), (12, 0.8125)], ids=["stride", "counter"])
def test_more_frames_than_workgroups(cap, scale):
    """5000 frames of B on far fewer resident workgroups: a fixed stride at cap
    8, the stream's counter at cap 12; through the host entry point, then on a
    second stream of the same context, on the first and on the second again."""
    import torch
    c = case("B")
    y = _queue_frames(c)
    ref = c.ref("yq", y, cap, scale=scale)
    assert _early_and_capped(ref["iters"], cap)
    dec = c.dec
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


# ---- 7. exit rule and batch sizes -------------------------------------------------------------

def test_et_period_and_single_iteration():
    c = case("B")
    y = np.concatenate([_queue_frames(c)[:100], c.frames(*qc.TABLE["B"][2][:3])[:24]])
    ref = lref.decode(c.csr, c.plan, y, 50, et_period=5)
    assert (ref["iters"] % 5 == 0).all() and _early_and_capped(ref["iters"], 50)
    _eq(c.dec.decode_layered(y, max_iters=50, et_period=5, want_llr=True), ref, what="et_period 5")
    _eq(c.dec.decode_layered(y, max_iters=1, want_llr=True), lref.decode(c.csr, c.plan, y, 1),
        what="one iteration")


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(B):
    c = case("B")
    y = c.frames(*qc.TABLE["B"][2][:3])[:B]
    _eq(c.dec.decode_layered(y, scale=0.8125, max_iters=12, want_llr=True),
        lref.decode(c.csr, c.plan, y, 12, scale=0.8125))


# ---- 8. input forms ---------------------------------------------------------------------------

def test_strided_complex_negative_polarity():
    """Interleaved complex samples, windows sliding by one sample (cw_stride =
    elem_stride = 2) at polarity -1 through the host entry point; then a real
    stream with a frame stride wider than N."""
    c = case("B")
    N = c.dec.N
    B = 40
    base = -c.frames(111, 2, 3.0).reshape(-1)
    z = np.zeros(2 * base.size + 10, np.float32)
    z[10::2] = base
    z[11::2] = np.random.Generator(np.random.PCG64(10)).standard_normal(base.size)
    frames = np.stack([z[10::2][s:s + N] for s in range(B)])         # window 0 is a frame
    ref = lref.decode(c.csr, c.plan, frames, 10, scale=0.8125, polarity=-1.0)
    assert _early_and_capped(ref["iters"], 10)
    _eq(c.dec.decode_layered(z[10:], scale=0.8125, max_iters=10, polarity=-1.0, cw_stride=2,
                             elem_stride=2, B=B, want_llr=True), ref)
    wide = np.zeros((B, N + 8), np.float32)
    wide[:, :N] = frames
    _eq(c.dec.decode_layered(wide, scale=0.8125, max_iters=10, polarity=-1.0, cw_stride=N + 8,
                             want_llr=True), ref, what="cw_stride N + 8")


# ---- 9. a quasi-cyclic context is a full context ----------------------------------------------

def test_the_context_is_a_full_context():
    """Last in the file: after every layered decode above, the context's
    flooding routes equal the oracle, and the ring refusal is the usual one."""
    import ldpc_ece535a as L
    from oracle import oracle as orc
    c = case("A")
    M, N, rp, ci = c.csr
    y = c.frames(*qc.TABLE["A"][2][:3])
    for method in (0, 1):
        _eq(c.dec.decode(y, method=method, max_iters=12),
            orc.decode_batch_sparse(method, rp, ci, M, N, y, 12, nthreads=16),
            what="method %d" % method)
    e = case("E")                                    # a small-code context: the ring's kind
    assert e.dec.path == 0
    ye = e.frames(*qc.TABLE["E"][2][:3])
    ref = e.ref("table", ye, 20, scale=1.0, precision=0)
    e.dec.ring_begin(method=1, max_iters=20)
    try:
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*ring"):
            e.dec.decode_layered(ye, max_iters=20)
    finally:
        e.dec.ring_end()
    e.dec.synchronize()
    _eq(e.dec.decode_layered(ye, max_iters=20, want_llr=True), ref, what="after the ring session")
