"""GPU parity of the fixed-point layered decoder (ldpc_decode_layered_q8*,
csrc/ldpc_layered.hip): int8 check messages and int16 posteriors in LDS, on
the circulant route (a quasi-cyclic context under its block rows) and on the
per-edge table route (any other context or plan).

Every comparison is against the numpy restatement of the contract
(tests/layered_q8_ref.py), never against a kernel: bits, packed bytes,
iteration counts, syndrome weights and the posteriors, all for equality.  The
codes are synthetic (tests/qc_cases.py, tests/shape_cases.py,
layered_q8_ref.large_base / boundary_base)."""
import numpy as np
import pytest

import layered_q8_ref as q8
import layered_ref as lref
import qc_cases as qc
from shape_cases import degree_limit_code, same_bits

pytestmark = pytest.mark.gpu

KEYS = q8.KEYS


def _eq(out, ref, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))
    if "llr" in out:
        same_bits(out["llr"], ref["llr"], what=what)


def _early_and_capped(iters, cap):
    return (iters < cap).any() and (iters == cap).any()


class _Case:
    """A code, a decoder for it and restatement results computed once."""

    def __init__(self, name=None, base=None, Z=None, csr=None, **kw):
        import ldpc_ece535a as L
        if csr is not None:
            self.csr, self.base = csr, None
            self.dec = L.Decoder(csr=csr, **kw)
            self.plan = lref.first_fit(csr)
        else:
            self.base, self.Z = qc.base_of(name) if base is None else (base, Z)
            L.plan_qc_q8(self.base, self.Z)                     # fails here without the feature
            self.csr = L.plan_qc(self.base, self.Z, precision=L.PREC_F32)["csr"]
            self.dec = L.Decoder(qc=(self.base, self.Z), **kw)
            self.plan = qc.block_rows(self.base.shape[0], self.Z)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def frames(self, fseed, B, db):
        return self.memo(("y", fseed, B, db), lambda: qc.frames(self.csr, fseed, B, db))

    def ref(self, key, y, cap, plan=None, **kw):
        return self.memo((key, cap, plan is None, tuple(sorted(kw.items()))), lambda: q8.decode(
            self.csr, self.plan if plan is None else plan, y, cap, **kw))


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


# name -> fseed, B, dB, cap: by the restatement, frames that stop early and
# frames that run to the cap at num 16 and at num 13 (asserted below)
RUNS = {"A": (101, 96, 2.0, 20), "B": (102, 96, 2.0, 20), "C": (103, 32, 5.0, 15),
        "D": (104, 16, 3.0, 12), "E": (105, 64, 1.0, 20), "F": (106, 8, 6.0, 10),
        "G": (107, 64, 5.0, 20)}


def _special(c, name):
    fseed, B, db, cap = RUNS[name]

    def make():
        y = c.frames(fseed, B, db).copy()
        if c.csr[1] >= 404:
            qc.plant_special(y)
        else:                                    # the same samples at columns a short code has
            y[::7, 3] = np.inf
            y[1::5, 10] = -np.inf
            y[2::9, 20] = np.nan
            y[3::4, 30:34] = 0.0
            y[1::8, 34:38] = -0.0
        return q8.plant_ties(y, 8.0)
    return c.memo("special", make)


# ---- 1. the circulant route --------------------------------------------------------------

@pytest.mark.parametrize("num", [16, 13])
@pytest.mark.parametrize("name", list("ABCDEFG"))
def test_circulant_cases(name, num):
    """A: Z = 64.  B: Z = 27, below a wave.  C: rows of 11..17 places.  D: six
    waves.  E: Z = 1.  F: 1024 threads.  G: rows of 32, 23, 12 and 1 places.
    Special samples (+-inf, NaN, +-0.0, ties at +-0.5, +-1.5, +-127.5) planted."""
    c = case(name)
    cap = RUNS[name][3]
    y = _special(c, name)
    ref = c.ref("special", y, cap, num=num, llr_scale=8.0)
    assert _early_and_capped(ref["iters"], cap), np.bincount(ref["iters"])
    _eq(c.dec.decode_layered_q8(y, num=num, llr_scale=8.0, max_iters=cap, want_llr=True), ref)


# ---- 2. the table route ------------------------------------------------------------------

def test_table_n720_first_fit():
    c = _Case(csr=lref.ira_code(360, 720, 1))
    assert (c.dec.layers == c.plan).all()
    y = q8.plant_ties(qc.plant_special(lref.noisy(c.csr, 64, 2.0, 5)), 8.0)
    for num in (16, 13):
        ref = q8.decode(c.csr, c.plan, y, 20, num=num)
        assert _early_and_capped(ref["iters"], 20)
        _eq(c.dec.decode_layered_q8(y, num=num, max_iters=20, want_llr=True), ref, "num %d" % num)
    c.dec.close()


def test_table_degree_limits():
    """A row of degree 32, one-row layers, a row and a column of degree 1, a
    column of degree 16."""
    csr, H = degree_limit_code()
    assert H.sum(axis=1).max() == 32 and H.sum(axis=0).max() == 16
    c = _Case(csr=csr, onchip=True)
    rng = np.random.Generator(np.random.PCG64(41))
    y = (-1.0 + np.sqrt(10 ** (-3.0 / 10)) * rng.standard_normal((64, 120))).astype(np.float32)
    for num in (16, 13):
        ref = q8.decode(csr, c.plan, y, 20, num=num)
        assert _early_and_capped(ref["iters"], 20)
        assert np.abs(ref["llr"]).max() <= 127 * 17
        _eq(c.dec.decode_layered_q8(y, num=num, max_iters=20, want_llr=True), ref, "num %d" % num)
    c.dec.close()


@pytest.mark.parametrize("name", ["B", "C"])
def test_table_route_on_a_qc_context(name):
    """LDPC_FLAG_QC_TABLES keeps the block rows and runs the table kernel: the
    restatement's outputs, hence the circulant kernel's."""
    c = case(name)
    cap = RUNS[name][3]
    y = _special(c, name)
    ref = c.ref("special", y, cap, num=13, llr_scale=8.0)
    tab = _Case(name, qc_tables=True)
    assert (tab.dec.layers == c.plan).all()
    a = c.dec.decode_layered_q8(y, num=13, max_iters=cap, want_llr=True)
    b = tab.dec.decode_layered_q8(y, num=13, max_iters=cap, want_llr=True)
    _eq(a, ref, "circulant kernel")
    _eq(b, ref, "table kernel")
    _eq(a, b, "circulant vs table kernel")
    tab.dec.close()


def test_table_route_with_tables_in_l2():
    """The table kernel with its tables left in global memory: Z = 1024, mb = 4,
    N = 16384, E = 44032 <= 65535 under the block rows.  The frame fits in LDS;
    the frame and the tables together do not, so nothing is staged."""
    import ldpc_ece535a as L
    base = q8.large_base(16)
    c = _Case("big16t", base, 1024, qc_tables=True)
    M, N, E, NL = c.csr[0], c.csr[1], c.csr[3].size, base.shape[0]
    assert (M, N, E, NL) == (4096, 16384, 44032, 4)

    def a16(x):
        return (x + 15) & ~15
    frame = a16(2 * N) + a16(E) + 128
    tables = a16(4 * M) + a16(2 * E) + a16(2 * M) + a16(4 * (NL + 1))
    assert frame == L.plan_qc_q8(base, 1024)["lds_bytes"] == 76928
    assert frame <= 160 * 1024 < frame + tables == 189600
    assert (c.dec.layers == c.plan).all()
    y = c.frames(136, 8, 3.0)
    for num in (16, 13):
        _eq(c.dec.decode_layered_q8(y, num=num, max_iters=5, want_llr=True),
            q8.decode(c.csr, c.plan, y, 5, num=num), "num %d" % num)
    c.dec.close()


def test_change_of_plan_between_decodes():
    """set_layers(first fit) on a quasi-cyclic context: the table kernel; back
    to the block rows: the circulant kernel again."""
    import ldpc_ece535a as L
    c = case("A")
    y = _special(c, "A")
    rows = c.ref("special", y, 20, num=16, llr_scale=8.0)
    first_fit = L.plan_layers_q8(c.csr)["layer_of_row"]
    assert (first_fit == lref.first_fit(c.csr)).all() and (first_fit != c.plan).any()
    ref = q8.decode(c.csr, first_fit, y, 20)
    assert (ref["iters"] != rows["iters"]).any() or (ref["llr"] != rows["llr"]).any()
    _eq(c.dec.decode_layered_q8(y, max_iters=20, want_llr=True), rows, "block rows")
    try:
        c.dec.set_layers(first_fit)
        _eq(c.dec.decode_layered_q8(y, max_iters=20, want_llr=True), ref, "first fit")
    finally:
        c.dec.set_layers(None)
    _eq(c.dec.decode_layered_q8(y, max_iters=20, want_llr=True), rows, "block rows restored")


# ---- 3. codes the float decoder refuses --------------------------------------------------

def test_larger_than_float():
    import ldpc_ece535a as L
    c = _Case("big12", q8.large_base(12), 1024)
    y = c.frames(132, 8, 3.0)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*bytes of LDS"):
        c.dec.decode_layered(y, max_iters=5, precision=L.PREC_F32)
    _eq(c.dec.decode_layered_q8(y, max_iters=5, want_llr=True),
        q8.decode(c.csr, c.plan, y, 5), "N = 12288, E = 31744")
    c.dec.close()


def test_e_past_16_bits():
    import ldpc_ece535a as L
    base = q8.large_base(24)
    c = _Case("big24", base, 1024)
    assert c.csr[3].size == 68608
    y = c.frames(144, 8, 3.0)
    _eq(c.dec.decode_layered_q8(y, max_iters=5, want_llr=True),
        q8.decode(c.csr, c.plan, y, 5), "E = 68608")
    c.dec.close()
    tab = _Case("big24t", base, 1024, qc_tables=True)
    with pytest.raises(L.LdpcError, match=r"LDPC_EUNSUPPORTED.*117888 bytes.*E must be <= 65535"):
        tab.dec.decode_layered_q8(y, max_iters=5)
    tab.dec.close()


def test_lds_boundary():
    import ldpc_ece535a as L
    inside = _Case("inside", q8.boundary_base(63), 1024)
    y = inside.frames(130, 2, 3.0)
    _eq(inside.dec.decode_layered_q8(y, max_iters=3, want_llr=True),
        q8.decode(inside.csr, inside.plan, y, 3), "162944 bytes")
    inside.dec.close()
    beyond = _Case("beyond", q8.boundary_base(64), 1024)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*163968 bytes of LDS"):
        beyond.dec.decode_layered_q8(beyond.frames(130, 2, 3.0), max_iters=3)
    beyond.dec.close()


# ---- 4. the frame queue ------------------------------------------------------------------

QUEUE_B = 20000      # case E's frame is 320 bytes: a device holds at most 32 workgroups per CU


@pytest.mark.parametrize("cap,num", [(8, 16), (12, 13)], ids=["stride", "counter"])
def test_more_frames_than_workgroups(cap, num):
    """20000 frames of E (N = 40) on fewer resident workgroups: a fixed stride
    at cap 8, the stream's counter at cap 12; through the host entry point, then
    on a second stream of the same context, on the first and on the second again."""
    import torch
    c = case("E")
    B = QUEUE_B
    assert B > 32 * torch.cuda.get_device_properties(0).multi_processor_count
    y = c.frames(108, B, 4.0)
    ref = c.ref("yq", y, cap, num=num, llr_scale=8.0)
    assert _early_and_capped(ref["iters"], cap)
    dec = c.dec
    _eq(dec.decode_layered_q8(y, num=num, max_iters=cap, want_llr=True), ref)
    d_y = torch.from_numpy(y).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (side.cuda_stream, None, side.cuda_stream):
        pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
        bt = torch.zeros((B, dec.N), dtype=torch.uint8, device="cuda")
        it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        sy = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        po = torch.zeros((B, dec.N), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_layered_q8_device(d_y.data_ptr(), B, pk.data_ptr(), num=num, max_iters=cap,
                                     d_bits=bt.data_ptr(), d_iters=it.data_ptr(),
                                     d_synd=sy.data_ptr(), d_llr=po.data_ptr(), stream=stream)
        side.synchronize()
        dec.synchronize()
        _eq(dict(packed=pk.cpu().numpy(), bits=bt.cpu().numpy(), iters=it.cpu().numpy(),
                 synd=sy.cpu().numpy(), llr=po.cpu().numpy()), ref, what="stream %r" % (stream,))


# ---- 5. entry-point behaviour ------------------------------------------------------------

def test_et_period_and_single_iteration():
    c = case("B")
    y = np.concatenate([c.frames(108, 40, 4.0), c.frames(102, 24, 2.0)])
    ref = q8.decode(c.csr, c.plan, y, 50, et_period=5)
    assert (ref["iters"] % 5 == 0).all() and _early_and_capped(ref["iters"], 50)
    assert np.unique(ref["iters"]).size >= 3
    _eq(c.dec.decode_layered_q8(y, max_iters=50, et_period=5, want_llr=True), ref, "et_period 5")
    _eq(c.dec.decode_layered_q8(y, max_iters=1, want_llr=True), q8.decode(c.csr, c.plan, y, 1),
        "one iteration")


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(B):
    c = case("B")
    y = c.frames(102, 96, 2.0)[:B]
    _eq(c.dec.decode_layered_q8(y, num=13, max_iters=12, want_llr=True),
        q8.decode(c.csr, c.plan, y, 12, num=13))


def test_strided_complex_negative_polarity():
    """Interleaved complex samples, windows sliding by one sample (cw_stride =
    elem_stride = 2) at polarity -1 through the host entry point."""
    c = case("B")
    N = c.dec.N
    B = 40
    base = -c.frames(111, 2, 3.0).reshape(-1)
    z = np.zeros(2 * base.size + 10, np.float32)
    z[10::2] = base
    z[11::2] = np.random.Generator(np.random.PCG64(10)).standard_normal(base.size)
    frames = np.stack([z[10::2][s:s + N] for s in range(B)])         # window 0 is a frame
    ref = q8.decode(c.csr, c.plan, frames, 10, num=13, llr_scale=4.0, polarity=-1.0)
    assert _early_and_capped(ref["iters"], 10)
    _eq(c.dec.decode_layered_q8(z[10:], num=13, llr_scale=4.0, max_iters=10, polarity=-1.0,
                                cw_stride=2, elem_stride=2, B=B, want_llr=True), ref)


def test_float_decodes_are_unchanged_around_a_q8_decode():
    """One context, one plan, shared device tables: float, q8, float."""
    c = case("A")
    y = _special(c, "A")
    want = lref.decode(c.csr, c.plan, y, 20, scale=0.8125, precision=1)
    before = c.dec.decode_layered(y, scale=0.8125, max_iters=20, precision=1, want_llr=True)
    _eq(c.dec.decode_layered_q8(y, num=13, max_iters=20, want_llr=True),
        c.ref("special", y, 20, num=13, llr_scale=8.0))
    after = c.dec.decode_layered(y, scale=0.8125, max_iters=20, precision=1, want_llr=True)
    _eq(before, want, "before")
    _eq(after, want, "after")
    _eq(after, before, "after vs before")


def test_refusals():
    import ldpc_ece535a as L
    c = case("E")
    y = c.frames(105, 4, 1.0)
    for num in (0, 17, -1):
        with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*num must be in \[1, 16\]"):
            c.dec.decode_layered_q8(y, num=num, max_iters=5)
    for s in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*llr_scale"):
            c.dec.decode_layered_q8(y, llr_scale=s, max_iters=5)
    assert c.dec.path == 0                           # a small-code context: the ring's kind
    c.dec.ring_begin(method=1, max_iters=20)
    try:
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*ring"):
            c.dec.decode_layered_q8(y, num=0, max_iters=5)      # the ring is named first
    finally:
        c.dec.ring_end()
    c.dec.synchronize()
    _eq(c.dec.decode_layered_q8(y, max_iters=5, want_llr=True), q8.decode(c.csr, c.plan, y, 5),
        "after the refusals")


def test_ber_sweep_q8_curve():
    import ldpc_ece535a as L
    from ldpc_ece535a import ber
    dec = L.Decoder()
    five = ber.sweep(dec, [2.0, 8.0], frames=30, iterations=5, seed=3, layered_scale=0.8125)
    six = ber.sweep(dec, [2.0, 8.0], frames=30, iterations=5, seed=3, layered_scale=0.8125,
                    layered_q8=(13, 8.0))
    assert list(six) == list(five) + [ber.LAYERED_Q8] and all(six[n] == five[n] for n in five)
    fix = six[ber.LAYERED_Q8]
    assert len(fix["ber"]) == len(fix["fer"]) == 2 and all(0.0 <= v <= 1.0 for v in fix["ber"])
    assert fix["ber"][1] <= fix["ber"][0] and all(0 <= v <= 30 for v in fix["fer"])
    assert "ber5=[" in ber.octave([2.0, 8.0], six) and "ber5" not in ber.octave([2.0, 8.0], five)
    dec.close()
