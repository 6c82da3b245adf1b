"""GPU: rate matching on the device (ldpc_rate_match_device,
ldpc_rate_recover_device: ldpc_aux.hip) against the host functions, and the
layered decodes whose frame load recovers the samples itself
(ldpc_decode_layered*_rm*: ldpc_layered.hip load_frame_rm) against the numpy
restatements -- tests/rate_match_ref.py for the recovery, then
tests/layered_ref.py / tests/layered_q8_ref.py for the decode of -recover(rx) --
bit for bit: bits, packed bytes, iteration counts, syndrome weights and the
posteriors as bit patterns.  The patterns are tests/rate_match_cases.py's."""
import numpy as np
import pytest

import layered_q8_ref as q8ref
import layered_ref as lref
import rate_match_cases as rc
import rate_match_ref as rm
from shape_cases import same_bits

pytestmark = pytest.mark.gpu

KEYS = lref.KEYS
TINY = 2.0 ** -100
B = 48
PAD = 5            # rx_stride = sum E + PAD, the gap filled with 3e38


class _Case:
    """A pattern's code, its contexts (the circulant route and, on demand, the
    per-edge tables) and what the restatements computed, once."""

    def __init__(self, name):
        self.name = name
        self.case = rc.CASES[name]
        self.csr, self.plan, self.qc = rc.code_of(self.case)
        self.M, self.N = self.case["M"], self.case["N"]
        self.pattern, self.tx = self.case["pattern"], self.case["tx"]
        self._dec = {}
        self._memo = {}

    def dec(self, route="circ"):
        import ldpc_ece535a as L
        if route not in self._dec:
            if self.qc is None:
                d = L.Decoder(csr=self.csr)
                d.set_layers(self.plan)
            else:
                d = L.Decoder(qc=self.qc, qc_tables=route == "tables")
            d.set_rate_match(*self.pattern)         # fails here without the feature
            self._dec[route] = d
        return self._dec[route]

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def rx(self, db, seed, polarity=1.0):
        """(cw, rx): noisy transmissions with the special samples planted; for
        polarity -1 the channel's samples negated, so the decode sees the same."""
        def make():
            cw, rx = rc.received(self.case, self.csr, B, db, seed)
            return cw, rc.plant_special(np.float32(polarity) * rx)
        return self.memo(("rx", db, seed, polarity), make)

    def lci(self, db, seed, polarity, unreceived):
        return self.memo(("lci", db, seed, polarity, unreceived), lambda: rm.recover(
            self.M, self.N, self.pattern, self.tx, self.rx(db, seed, polarity)[1], polarity,
            unreceived))

    def ref(self, arith, kw, cap, db, seed, polarity, unreceived):
        """The restatement's decode of y = -recover(rx), at polarity 1."""
        def run():
            y = -self.lci(db, seed, polarity, unreceived)
            if arith == "q8":
                return q8ref.decode(self.csr, self.plan, y, cap, **kw)
            return lref.decode(self.csr, self.plan, y, cap, precision=int(arith == "f32"), **kw)
        return self.memo(("ref", arith, tuple(sorted(kw.items())), cap, db, seed, polarity,
                          unreceived), run)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _eq(out, ref, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))
    same_bits(out["llr"], ref["llr"], what=what)


def _early_and_capped(iters, cap):
    return (iters < cap).any() and (iters == cap).any()


def _fused(dec, arith, kw, cap, rx, tx, polarity, unreceived, device=False):
    """The fused decode of rx (B, sum E) at a stride of sum E + PAD."""
    wide = rc.strided(rx, PAD)
    common = dict(max_iters=cap, polarity=polarity, unreceived_lci=unreceived,
                  rx_stride=wide.shape[1], **kw)
    if not device:
        if arith == "q8":
            return dec.decode_layered_q8_rm(wide, tx, B=rx.shape[0], want_llr=True, **common)
        return dec.decode_layered_rm(wide, tx, precision=int(arith == "f32"), B=rx.shape[0],
                                     want_llr=True, **common)
    import torch
    n = rx.shape[0]
    dev = torch.device("cuda", 0)
    d_rx = torch.from_numpy(wide).to(dev)
    o = dict(packed=torch.zeros((n, dec.KB), dtype=torch.uint8, device=dev),
             bits=torch.zeros((n, dec.N), dtype=torch.uint8, device=dev),
             iters=torch.zeros(n, dtype=torch.int32, device=dev),
             synd=torch.zeros(n, dtype=torch.int32, device=dev),
             llr=torch.zeros((n, dec.N), dtype=torch.float32, device=dev))
    ptrs = dict(d_bits=o["bits"].data_ptr(), d_iters=o["iters"].data_ptr(),
                d_synd=o["synd"].data_ptr(), d_llr=o["llr"].data_ptr())
    if arith == "q8":
        dec.decode_layered_q8_rm_device(d_rx.data_ptr(), n, tx, o["packed"].data_ptr(), **common,
                                        **ptrs)
    else:
        dec.decode_layered_rm_device(d_rx.data_ptr(), n, tx, o["packed"].data_ptr(),
                                     precision=int(arith == "f32"), **common, **ptrs)
    dec.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---- 1. the device selector and combiner against the host functions ------------------------

@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_selector_and_combiner_equal_the_host(name):
    import torch
    from ldpc_ece535a import _capi
    c = case(name)
    dec = c.dec()
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(31))
    n = 9
    bits = rng.integers(0, 2, (n, c.N), np.uint8)
    d_bits = torch.from_numpy(np.where(bits == 1, 0x03, 0xFE).astype(np.uint8)).to(dev)
    for k0, E in c.tx:
        d_out = torch.full((n, E + 3), 0xAA, dtype=torch.uint8, device=dev)
        dec.rate_match_device(d_bits.data_ptr(), n, k0, E, d_out.data_ptr(), out_stride=E + 3)
        dec.synchronize()
        out = d_out.cpu().numpy()
        np.testing.assert_array_equal(out[:, :E], _capi.rate_match(c.M, c.N, *c.pattern, k0, E, bits))
        assert (out[:, E:] == 0xAA).all(), "wrote beyond E"
    rx = rc.plant_special(rng.standard_normal((n, rc.total(c.case))).astype(np.float32))
    for pol, un in ((1.0, TINY), (-1.0, 0.0)):
        wide = rc.strided(rx, PAD)
        d_y = torch.full((n + 1, c.N), 7.0, dtype=torch.float32, device=dev)
        dec.rate_recover_device(torch.from_numpy(wide).to(dev).data_ptr(), n, c.tx, d_y.data_ptr(),
                                polarity=pol, unreceived_lci=un, rx_stride=wide.shape[1])
        dec.synchronize()
        y = d_y.cpu().numpy()
        host = _capi.rate_recover(c.M, c.N, *c.pattern, c.tx, wide, polarity=pol,
                                  unreceived_lci=un, rx_stride=wide.shape[1], B=n)
        same_bits(y[:n], host, what="%s polarity %g" % (name, pol))
        same_bits(host, -rm.recover(c.M, c.N, c.pattern, c.tx, rx, pol, un), what="host")
        assert (y[n] == 7.0).all(), "wrote beyond B frames"


# ---- 2. the fused decodes against the restatements -----------------------------------------

# id: (case, arithmetic, its parameters, cap, dB, seed, polarity, unreceived_lci, routes).
# Float runs that check the syndrome every third iteration take 2**-10 for the
# unreceived columns: with 2**-100 the restatement stops a frame of these
# patterns after its first iteration or never (DESIGN section 7f says why), so
# a check at iteration 3 finds none.
Q8 = dict(num=13, llr_scale=8.0)
SMALL = 2.0 ** -10
BOTH = ("circ", "tables")
RUNS = {
    "b-f64": ("b", "f64", dict(scale=0.8125), 50, 9.0, 201, 1.0, TINY, BOTH),
    "b-f64-et3": ("b", "f64", dict(scale=0.8125, et_period=3), 50, 9.0, 201, 1.0, SMALL, ("circ",)),
    "b-f32-plain-neg": ("b", "f32", dict(scale=1.0), 50, 9.0, 201, -1.0, TINY, BOTH),
    "b-q8": ("b", "q8", Q8, 50, 9.0, 201, 1.0, TINY, BOTH),
    "c-f64-et3": ("c", "f64", dict(scale=0.8125, et_period=3), 50, 9.0, 202, 1.0, SMALL, BOTH),
    "c-f32-plain-et3": ("c", "f32", dict(scale=1.0, et_period=3), 50, 9.0, 202, 1.0, SMALL,
                        ("circ",)),
    "c-f32": ("c", "f32", dict(scale=0.8125), 50, 9.0, 202, 1.0, TINY, ("circ",)),
    "c-q8-et3": ("c", "q8", dict(et_period=3, **Q8), 50, 9.0, 202, 1.0, TINY, ("circ",)),
    "c3-f32-plain": ("c3", "f32", dict(scale=1.0), 50, 9.0, 203, 1.0, TINY, ("circ",)),
    "d-f64": ("d", "f64", dict(scale=0.8125), 50, 9.0, 204, 1.0, TINY, ("circ",)),
    "d-q8-neg": ("d", "q8", Q8, 50, 9.0, 204, -1.0, TINY, BOTH),
    "d2-f32": ("d2", "f32", dict(scale=0.8125), 50, 9.0, 205, 1.0, TINY, ("circ",)),
    "e-f64": ("e", "f64", dict(scale=0.8125), 50, 9.0, 206, 1.0, TINY, BOTH),
    "e-f64-zero": ("e", "f64", dict(scale=0.8125), 50, 9.0, 206, 1.0, 0.0, ("circ",)),
    "e-q8-zero": ("e", "q8", Q8, 50, 9.0, 206, 1.0, 0.0, ("circ",)),
    "f-f32": ("f", "f32", dict(scale=0.8125), 10, 9.0, 207, 1.0, TINY, ("circ",)),
    "f2-f32": ("f2", "f32", dict(scale=0.8125), 10, 9.0, 207, 1.0, TINY, ("circ",)),
    "g-f64": ("g", "f64", dict(scale=0.8125), 50, 9.0, 208, 1.0, TINY, ("circ",)),
    "g-f32-et3": ("g", "f32", dict(scale=0.8125, et_period=3), 50, 9.0, 208, 1.0, TINY, ("circ",)),
    "g-q8": ("g", "q8", Q8, 50, 9.0, 208, 1.0, TINY, ("circ",)),
}
# (f) sends K positions for K information bits: every frame runs to the cap
ALL_CAPPED = {"f-f32"}


def reference_of(run):
    """(case, rx, ref) of a run: the restatement alone, no GPU."""
    name, arith, kw, cap, db, seed, pol, un, _ = RUNS[run]
    c = case(name)
    return c, c.rx(db, seed, pol)[1], c.ref(arith, kw, cap, db, seed, pol, un)


@pytest.mark.parametrize("run", sorted(RUNS))
def test_fused_decode(run):
    """Every run stops at least one frame early and takes at least one to the
    cap, by the restatement's own output -- but (f), whose buffer is as long as
    the information part: there every frame runs to the cap, and (f2), the same
    code with one block column punctured, stands in.  The first route is also
    run through the device entry point."""
    name, arith, kw, cap, db, seed, pol, un, routes = RUNS[run]
    c, rx, ref = reference_of(run)
    if run in ALL_CAPPED:
        assert (ref["iters"] == cap).all()
    else:
        assert _early_and_capped(ref["iters"], cap), (ref["iters"].min(), ref["iters"].max())
    for route in routes:
        dec = c.dec(route)
        _eq(_fused(dec, arith, kw, cap, rx, c.tx, pol, un), ref, what="%s %s" % (run, route))
    _eq(_fused(c.dec(routes[0]), arith, kw, cap, rx, c.tx, pol, un, device=True), ref,
        what="%s device" % run)


def test_zero_for_the_unreceived_silences_their_rows():
    """What the header says 0.0 does to the float decoder on (b): the decode is
    still the contract's, bit for bit, and no frame leaves before the cap; with
    the default every frame of the same noiseless batch decodes at once."""
    c = case("b")
    cw, _ = rc.codewords(c.case, c.csr, B, 209)
    cols = rm.columns(c.M, c.N, c.pattern, c.tx)
    rx = (2.0 * cw[:, cols] - 1.0).astype(np.float32)
    for un, iters in ((0.0, 8), (TINY, 1)):
        y = -rm.recover(c.M, c.N, c.pattern, c.tx, rx, 1.0, un)
        ref = lref.decode(c.csr, c.plan, y, 8, scale=0.8125)
        assert (ref["iters"] == iters).all()
        _eq(_fused(c.dec(), "f64", dict(scale=0.8125), 8, rx, c.tx, 1.0, un), ref, what=str(un))
    assert (ref["synd"] == 0).all() and (ref["bits"] == cw).all()


# ---- 3. against the library's own plain paths ----------------------------------------------

def test_identity_equals_the_plain_decode():
    """Pattern (0, 0, 0), one transmission of N: decode_layered_rm is
    decode_layered on the permuted samples, NaN and -0.0 included."""
    c = case("a")
    dec = c.dec()
    y = rc.qc.plant_special(rc.qc.frames(c.csr, 210, B, 2.0))
    perm = rm.columns(c.M, c.N, c.pattern, c.tx)
    np.testing.assert_array_equal(perm, np.r_[c.M:c.N, 0:c.M])
    rx = y[:, perm]
    for arith, kw in (("f64", dict(scale=0.8125)), ("f32", dict(scale=1.0)), ("q8", Q8)):
        if arith == "q8":
            plain = dec.decode_layered_q8(y, max_iters=20, want_llr=True, **kw)
        else:
            plain = dec.decode_layered(y, max_iters=20, precision=int(arith == "f32"),
                                       want_llr=True, **kw)
        assert _early_and_capped(plain["iters"], 20)
        _eq(_fused(dec, arith, kw, 20, rx, c.tx, 1.0, TINY), plain, what=arith)


@pytest.mark.parametrize("run", ["b-f64", "c-q8-et3", "d2-f32", "g-f32-et3"])
def test_fused_equals_recover_then_decode(run):
    """rate_recover_device, then the plain device decode at polarity 1."""
    import torch
    name, arith, kw, cap, db, seed, pol, un, routes = RUNS[run]
    c, rx, ref = reference_of(run)
    dec = c.dec(routes[0])
    dev = torch.device("cuda", 0)
    wide = rc.strided(rx, PAD)
    d_y = torch.empty((B, c.N), dtype=torch.float32, device=dev)
    dec.rate_recover_device(torch.from_numpy(wide).to(dev).data_ptr(), B, c.tx, d_y.data_ptr(),
                            polarity=pol, unreceived_lci=un, rx_stride=wide.shape[1])
    dec.synchronize()
    y = d_y.cpu().numpy()
    if arith == "q8":
        two = dec.decode_layered_q8(y, max_iters=cap, want_llr=True, **kw)
    else:
        two = dec.decode_layered(y, max_iters=cap, precision=int(arith == "f32"), want_llr=True,
                                 **kw)
    _eq(two, ref, what="two steps")
    _eq(_fused(dec, arith, kw, cap, rx, c.tx, pol, un), two, what="fused")


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_round_trip_on_the_device(name):
    """encode_device -> rate_match_device per transmission -> noiseless BPSK ->
    the fused decode: the data comes back with syndrome 0."""
    import torch
    import ldpc_ece535a as L
    c = case(name)
    dec = c.dec()
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(211))
    data = rng.integers(0, 2, (B, dec.K), np.uint8)
    data[:, dec.K - c.pattern[1]:] = 0
    d_data = torch.from_numpy(data).to(dev)
    d_cw = torch.empty((B, dec.N), dtype=torch.uint8, device=dev)
    total = rc.total(c.case)
    d_tx = torch.empty((B, total), dtype=torch.uint8, device=dev)
    dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr())
    off = 0
    for k0, E in c.tx:
        dec.rate_match_device(d_cw.data_ptr(), B, k0, E, d_tx.data_ptr() + off, out_stride=total)
        off += E
    dec.synchronize()
    d_rx = (2.0 * d_tx.to(torch.float32) - 1.0).contiguous()
    torch.cuda.synchronize()
    d_packed = torch.zeros((B, dec.KB), dtype=torch.uint8, device=dev)
    d_synd = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_bits = torch.zeros((B, dec.N), dtype=torch.uint8, device=dev)
    dec.decode_layered_rm_device(d_rx.data_ptr(), B, c.tx, d_packed.data_ptr(), scale=0.8125,
                                 max_iters=20, precision=L.PREC_F32, d_bits=d_bits.data_ptr(),
                                 d_synd=d_synd.data_ptr())
    dec.synchronize()
    assert (d_synd.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(d_bits.cpu().numpy(), d_cw.cpu().numpy())
    np.testing.assert_array_equal(d_packed.cpu().numpy(), np.packbits(data, axis=1))


def test_refusals_of_the_context_calls():
    import torch
    import ldpc_ece535a as L
    c = case("b")
    dec = c.dec()
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*punct must be <= K - filler = 284 \(got 300\)"):
        dec.set_rate_match(300, 40, 0)
    rx = np.zeros((1, 500), np.float32)
    assert dec.decode_layered_rm(rx, [(0, 473)], rx_stride=500, B=1)["iters"].shape == (1,)
    with pytest.raises(L.LdpcError, match=r"k0 must be in \[0, ncb = 594\) \(got 594\)"):
        dec.decode_layered_rm(rx, [(594, 10)], rx_stride=500, B=1)
    with pytest.raises(L.LdpcError, match=r"E must be in \[1, 16 S = 8864\] \(got 8865\)"):
        dec.decode_layered_q8_rm(rx, [(0, 8865)], rx_stride=500, B=1)
    with pytest.raises(L.LdpcError, match=r"rx_stride must be >= the sum of E = 473 \(got 472\)"):
        dec.decode_layered_rm(rx, [(0, 473)], rx_stride=472, B=1)
    with pytest.raises(L.LdpcError, match="unreceived_lci must not be NaN"):
        dec.decode_layered_rm(rx, [(0, 473)], rx_stride=500, B=1, unreceived_lci=float("nan"))
    with pytest.raises(L.LdpcError, match="input shorter than the frames read"):
        dec.decode_layered_rm(rx, [(0, 473)], rx_stride=500, B=2)
    with pytest.raises(L.LdpcError, match="scale must be finite"):
        dec.decode_layered_rm(rx, [(0, 473)], scale=1.5, rx_stride=500, B=1)
    d = torch.zeros(600, dtype=torch.float32, device="cuda:0")
    with pytest.raises(L.LdpcError, match=r"n_tx must be in \[1, 4\]"):
        dec.rate_recover_device(d.data_ptr(), 1, [(0, 10)] * 5, d.data_ptr())
    with pytest.raises(L.LdpcError, match="out_stride >= E"):
        dec.rate_match_device(d.data_ptr(), 1, 0, 10, d.data_ptr(), out_stride=9)
    dec.decode_layered_rm(rx, [(0, 473)], rx_stride=500, B=0)     # an empty batch is a no-op


def test_ber_sweep_of_a_rate_matched_code(tmp_path, capsys):
    """python -m ldpc_ece535a.ber --qc ... --rate-match 54,40,0 --tx 0:300,150:250: the six
    curves over the grid, every figure in range, the layered curves clean where
    the noise is negligible (30 dB: on the CPU the restatements decode all 64
    such frames of this code in two iterations, the float one with 2**-10 for
    the unsent columns -- with 2**-100 it decodes none), and
    the JSON's note on what BER and sigma mean here."""
    import json
    from ldpc_ece535a import ber
    out = tmp_path / "ber.json"
    rc_ = ber.main(["--qc", "4,8,24,27,3,1", "--layered", "0.8125", "--layered-q8", "13",
                    "--rate-match", "54,40,0", "--tx", "0:300,150:250", "--ebn0", "3,30",
                    "--unreceived-lci", str(2.0 ** -10),
                    "--frames", "64", "--iterations", "10", "--precision", "1", "--json", str(out)])
    assert rc_ == 0
    assert "LayeredMinSumQ8" in capsys.readouterr().out
    doc = json.loads(out.read_text())
    assert doc["rate_match"] == dict(punct=54, filler=40, ncb=0, tx=[[0, 300], [150, 250]],
                                     unreceived_lci=2.0 ** -10, note=ber.RATE_MATCH_NOTE)
    assert "no code-rate term" in ber.RATE_MATCH_NOTE and "all N" in ber.RATE_MATCH_NOTE
    res = doc["results"]
    assert set(res) == {"BPSK", "BitFlip", "LogDomainSimple", "SumProduct", ber.LAYERED,
                        ber.LAYERED_Q8}
    for name, r in res.items():
        print(name, r)
        assert len(r["ber"]) == len(r["fer"]) == 2
        assert all(0.0 <= v <= 1.0 for v in r["ber"]) and all(0 <= v <= 64 for v in r["fer"])
    for name in (ber.LAYERED, ber.LAYERED_Q8):
        assert res[name]["ber"][1] == 0.0 and res[name]["fer"][1] == 0, name
        assert res[name]["ber"][0] >= res[name]["ber"][1]
