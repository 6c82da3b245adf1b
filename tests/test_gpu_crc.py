"""GPU: the code-block CRC (include/ldpc_hip.h): the attach and check kernels
(ldpc_aux.hip) against the host functions, and the layered decodes that check
the CRC beside the syndrome (ldpc_layered.hip, ldpc_set_crc) against the numpy
restatements -- tests/crc_ref.py's decode_crc over tests/layered_ref.py /
tests/layered_q8_ref.py, behind tests/rate_match_ref.py for the fused decodes --
bit for bit: bits, packed bytes, iteration counts, syndrome weights, remainders
and the posteriors as bit patterns."""
import numpy as np
import pytest

import crc_ref as cr
import layered_q8_ref as q8ref
import layered_ref as lref
import qc_cases as qc
import rate_match_cases as rc
import rate_match_ref as rm
from shape_cases import same_bits

pytestmark = pytest.mark.gpu

KEYS = lref.KEYS + ("crc",)
Q8 = dict(num=13, llr_scale=8.0)
ARITH = {"f64": dict(scale=0.8125), "f32": dict(scale=0.8125), "q8": Q8}
SMALL = 2.0 ** -10
STOP_SEED = 500      # PCG64: the payloads first, then the noise


class _Code:
    """A code of tests/qc_cases.py (or the IRA code), its contexts by (route,
    pattern) and what the restatements computed, once."""

    def __init__(self, name):
        self.name = name
        self.csr, self.plan, self.qc = rc.code_of(dict(code=name))
        self.M, self.N = int(self.csr[0]), int(self.csr[1])
        self.K = self.N - self.M
        self._dec, self._memo = {}, {}

    def dec(self, route="circ", pattern=(0, 0, 0)):
        import ldpc_ece535a as L
        key = (route, pattern)
        if key not in self._dec:
            if self.qc is None:
                d = L.Decoder(csr=self.csr)
                d.set_layers(self.plan)
            else:
                d = L.Decoder(qc=self.qc, qc_tables=route == "tables")
            d.set_rate_match(*pattern)
            self._dec[key] = d
        return self._dec[key]

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def encode(self, info):
        from ldpc_ece535a import codes
        enc = codes.ira_encode if self.qc is None else codes.qc_encode
        return enc(self.csr, info).astype(np.uint8)

    def frames(self, crc, B, db, seed, filler=0):
        """(payload, cw, y): random payloads with the CRC attached, encoded,
        as noisy BPSK.  The payloads are drawn before the noise."""
        def make():
            rng = np.random.Generator(np.random.PCG64(seed))
            payload = rng.integers(0, 2, (B, self.K - filler - crc[0]), np.uint8)
            cw = self.encode(cr.attach(*crc, payload, self.K))
            y = 2.0 * cw - 1.0 + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(cw.shape)
            return payload, cw, y.astype(np.float32)
        return self.memo(("frames", crc, B, db, seed, filler), make)


_codes = {}


def code(name):
    if name not in _codes:
        _codes[name] = _Code(name)
    return _codes[name]


def _decode(dec, arith, y, cap, et_period=1):
    if arith == "q8":
        return dec.decode_layered_q8(y, max_iters=cap, et_period=et_period, want_llr=True, **Q8)
    return dec.decode_layered(y, max_iters=cap, et_period=et_period, want_llr=True,
                              precision=int(arith == "f32"), **ARITH[arith])


def _reference(c, arith, y, cap, crc, A, mode, et_period=1):
    if arith == "q8":
        return cr.decode_crc(q8ref.decode, c.csr, c.plan, y, cap, crc, A, mode, et_period, **Q8)
    return cr.decode_crc(lref.decode, c.csr, c.plan, y, cap, crc, A, mode, et_period,
                         precision=int(arith == "f32"), **ARITH[arith])


def _eq(out, ref, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))
    same_bits(out["llr"], ref["llr"], what=what)


# ---- 1. the attach and check kernels against the host --------------------------------------

KERNEL_CASES = {
    "E-crc6": ("E", (0, 0, 0), cr.CRC6),              # K = 20: fewer bits than a wave has lanes
    "B-b-crc24b": ("B", rc.CASES["b"]["pattern"], cr.CRC24B),   # A = 284, fillers split a circulant
    "F-crc24a": ("F", (0, 0, 0), cr.CRC24A),          # K = 4096
    "F-crc11": ("F", (0, 0, 0), cr.CRC11),
}


@pytest.mark.parametrize("B", [1, 48])
@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_attach_and_check_kernels_equal_the_host(name, B):
    import torch
    from ldpc_ece535a import _capi
    cname, pattern, crc = KERNEL_CASES[name]
    c = code(cname)
    dec = c.dec("circ", pattern)
    dec.set_crc(*crc)                                 # fails here without the feature
    filler = pattern[1]
    A = c.K - filler
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(51))
    payload = rng.integers(0, 2, (B, A - crc[0]), np.uint8)
    d_payload = torch.from_numpy(np.where(payload == 1, 0x03, 0xFE).astype(np.uint8)).to(dev)
    d_info = torch.full((B + 1, c.K), 0xAA, dtype=torch.uint8, device=dev)
    dec.crc_attach_device(d_payload.data_ptr(), B, d_info.data_ptr())
    dec.synchronize()
    info = d_info.cpu().numpy()
    host = _capi.crc_attach(c.M, c.N, filler, *crc, payload)
    np.testing.assert_array_equal(info[:B], host)
    np.testing.assert_array_equal(host, cr.attach(*crc, payload, c.K))
    assert (info[B] == 0xAA).all(), "wrote beyond B frames"
    # the check: attached blocks, one-bit errors, random blocks; the fillers' bits are not read
    blocks = host.copy()
    blocks[1::3, :A] ^= (np.arange(A)[None, :] == rng.integers(0, A, (B, 1))[1::3]).astype(np.uint8)
    blocks[2::3, :A] = rng.integers(0, 2, blocks[2::3, :A].shape, np.uint8)
    blocks[:, A:] = rng.integers(0, 2, blocks[:, A:].shape, np.uint8)
    d_packed = torch.from_numpy(np.packbits(blocks, axis=1)).to(dev)
    assert d_packed.shape == (B, dec.KB)
    d_rem = torch.full((B + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    dec.crc_check_device(d_packed.data_ptr(), B, d_rem.data_ptr() + 4)
    dec.synchronize()
    rem = d_rem.cpu().numpy().view(np.uint32)
    want = cr.remainder(*crc, blocks[:, :A])
    np.testing.assert_array_equal(rem[1:B + 1], want)
    assert rem[0] == 0x5A5A5A5A and rem[B + 1] == 0x5A5A5A5A, "wrote around the B remainders"
    assert (want[0::3] == 0).all() and (want[1::3] != 0).all()
    dec.set_crc(0)


# ---- 2. report mode: the plain decode and one more output ----------------------------------

@pytest.mark.parametrize("route", ["circ", "tables"])
@pytest.mark.parametrize("arith", ["f64", "f32", "q8"])
def test_report_mode_is_the_plain_decode(arith, route):
    c = code("B")
    dec = c.dec(route)
    (fseed, B, db, cap, _) = qc.TABLE["B"][2]
    y = c.memo("special", lambda: qc.plant_special(qc.frames(c.csr, fseed, B, db)))
    dec.set_crc(0)
    plain = _decode(dec, arith, y, cap)
    assert "crc" not in plain
    assert (plain["iters"] < cap).any() and (plain["iters"] == cap).any()
    dec.set_crc(*cr.CRC16, mode="report")
    out = _decode(dec, arith, y, cap)
    dec.set_crc(0)
    _eq(out, plain, keys=lref.KEYS, what="%s %s" % (arith, route))
    want = cr.remainder(*cr.CRC16, out["bits"][:, c.M:c.N])
    np.testing.assert_array_equal(out["crc"], want)
    assert out["crc"].dtype == np.uint32 and (want != 0).any()


# ---- 3. stop mode against decode_crc -------------------------------------------------------

def _stop_reference(arith, et):
    c = code("B")
    _, _, y = c.frames(cr.CRC16, 48, 2.0, STOP_SEED)
    return c.memo(("stop", arith, et),
                  lambda: _reference(c, arith, y, 20, cr.CRC16, c.K, "stop", et))


@pytest.mark.parametrize("et", [1, 3])
@pytest.mark.parametrize("arith", ["f32", "q8"])
def test_stop_mode(arith, et):
    """Code B, 48 frames of seed 500 with CRC16 attached, 2 dB, cap 20.  By the
    restatement alone, with et_period 1, at least 10 frames leave on the CRC
    with the syndrome still non-zero, and none passes with a wrong payload."""
    c = code("B")
    payload, cw, y = c.frames(cr.CRC16, 48, 2.0, STOP_SEED)
    ref1 = _stop_reference(arith, 1)
    on_crc = (ref1["crc"] == 0) & (ref1["synd"] > 0)
    print("frames that stop on the CRC with synd > 0:", int(on_crc.sum()))
    assert on_crc.sum() >= 10
    ref = _stop_reference(arith, et)
    passed = ref["crc"] == 0
    assert (ref["bits"][passed][:, c.M:c.M + payload.shape[1]] == payload[passed]).all(), \
        "a frame passes the CRC with a wrong payload"
    assert passed.any() and (~passed).any()
    for route in ("circ", "tables"):
        dec = c.dec(route)
        dec.set_crc(*cr.CRC16, mode="stop")
        out = _decode(dec, arith, y, 20, et)
        dec.set_crc(0)
        _eq(out, ref, what="%s et %d %s" % (arith, et, route))


# ---- 4. fused with rate matching -----------------------------------------------------------

@pytest.mark.parametrize("arith", ["f32", "q8"])
@pytest.mark.parametrize("name", ["b", "d"])
def test_stop_mode_fused_with_rate_matching(name, arith):
    """Patterns (b) and (d) of tests/rate_match_cases.py, CRC24B in the A = 284
    positions in front of the fillers: recover, then decode_crc."""
    case = rc.CASES[name]
    c = code("B")
    pattern, tx = case["pattern"], case["tx"]
    A = c.K - pattern[1]
    B, db, cap = 24, 6.0, 12
    payload, cw, _ = c.frames(cr.CRC24B, B, db, 520, filler=pattern[1])

    def received():
        rng = np.random.Generator(np.random.PCG64(521))
        x = 2.0 * cw[:, rm.columns(c.M, c.N, pattern, tx)] - 1.0
        return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)
    rx = c.memo(("rx", name), received)
    ref = c.memo(("fused", name, arith), lambda: _reference(
        c, arith, -rm.recover(c.M, c.N, pattern, tx, rx, 1.0, SMALL), cap, cr.CRC24B, A, "stop"))
    print(name, arith, "iters", np.bincount(ref["iters"]), "passed", int((ref["crc"] == 0).sum()))
    assert (ref["crc"] == 0).any()
    wide = rc.strided(rx, 5)
    dec = c.dec("circ", pattern)
    dec.set_crc(*cr.CRC24B, mode="stop")
    kw = dict(max_iters=cap, unreceived_lci=SMALL, rx_stride=wide.shape[1], B=B, want_llr=True)
    if arith == "q8":
        out = dec.decode_layered_q8_rm(wide, tx, **kw, **Q8)
    else:
        out = dec.decode_layered_rm(wide, tx, precision=1, **kw, **ARITH[arith])
    dec.set_crc(0)
    _eq(out, ref, what="%s %s" % (name, arith))


# ---- 5. shapes ------------------------------------------------------------------------------

# code, CRC, B, dB, cap, route: D six waves (the cross-wave XOR), F 1024 threads
# and four strides of positions, E A < 64, the IRA code on the table route with
# first-fit layers
SHAPES = {
    "D": ("D", cr.CRC24A, 8, 4.0, 6, "circ"),
    "F": ("F", cr.CRC24C, 8, 6.0, 4, "circ"),
    "E": ("E", cr.CRC11, 48, 3.0, 10, "circ"),
    "E-tables": ("E", cr.CRC6, 48, 3.0, 10, "tables"),
    rc.IRA: (rc.IRA, cr.CRC16, 16, 2.5, 10, "circ"),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stop_mode_shapes(shape):
    name, crc, B, db, cap, route = SHAPES[shape]
    c = code(name)
    _, _, y = c.frames(crc, B, db, 530)
    ref = _reference(c, "f32", y, cap, crc, c.K, "stop")
    print(shape, "iters", np.bincount(ref["iters"]), "passed", int((ref["crc"] == 0).sum()))
    dec = c.dec(route)
    dec.set_crc(*crc, mode="stop")
    out = _decode(dec, "f32", y, cap)
    dec.set_crc(0)
    _eq(out, ref, what=shape)


# ---- 6. around the outputs -----------------------------------------------------------------

def test_results_array_and_turning_the_crc_off():
    import ctypes
    import torch
    import ldpc_ece535a as L
    from ldpc_ece535a import _capi
    c = code("B")
    dec = c.dec()
    _, _, y = c.frames(cr.CRC16, 48, 2.0, STOP_SEED)
    dec.set_crc(0)
    before = _decode(dec, "f32", y, 20)
    ref = _stop_reference("f32", 1)
    dec.set_crc(*cr.CRC16, mode="stop")
    # two decodes of different B on one context: the array grows
    small = _decode(dec, "f32", y[:8], 20)
    np.testing.assert_array_equal(small["crc"], ref["crc"][:8])
    big = _decode(dec, "f32", y, 20)
    _eq(big, ref, what="after growing")
    # n < B, into the middle of a host buffer
    buf = np.full(12, 0xDEADBEEF, np.uint32)
    lib = _capi.lib()
    assert lib.ldpc_crc_results(dec.handle, buf[2:].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                5) == 0
    np.testing.assert_array_equal(buf[2:7], ref["crc"][:5])
    assert (buf[:2] == 0xDEADBEEF).all() and (buf[7:] == 0xDEADBEEF).all()
    with pytest.raises(L.LdpcError, match=r"n must be in \[0, 48\].*\(got 49\)"):
        dec.crc_results(49)
    # the device entry point, and the device array
    dev = torch.device("cuda", 0)
    d_y = torch.from_numpy(y[:8]).to(dev)
    d_packed = torch.zeros((8, dec.KB), dtype=torch.uint8, device=dev)
    d_iters = torch.zeros(8, dtype=torch.int32, device=dev)
    dec.decode_layered_device(d_y.data_ptr(), 8, d_packed.data_ptr(), precision=1, max_iters=20,
                              d_iters=d_iters.data_ptr(), **ARITH["f32"])
    np.testing.assert_array_equal(dec.crc_results(8), ref["crc"][:8])
    np.testing.assert_array_equal(d_iters.cpu().numpy(), ref["iters"][:8])
    np.testing.assert_array_equal(d_packed.cpu().numpy(), ref["packed"][:8])
    assert dec.crc_results_device()
    with pytest.raises(L.LdpcError, match=r"n must be in \[0, 8\]"):
        dec.crc_results(9)
    # off again: the parent's decode, and no "crc"
    dec.set_crc(0)
    after = _decode(dec, "f32", y, 20)
    assert "crc" not in after
    _eq(after, before, keys=lref.KEYS, what="off again")
    assert (before["iters"] != ref["iters"]).any()
    with pytest.raises(L.LdpcError, match="no CRC is set"):
        dec.crc_results(1)


def test_ber_sweep_with_a_crc(tmp_path, capsys):
    """python -m ldpc_ece535a.ber --qc ... --crc CRC16:stop: every curve reports
    the frames that passed, the undetected errors and the mean iterations; where
    the noise is negligible the layered curves pass every frame after their
    first iteration."""
    import json
    from ldpc_ece535a import ber
    out = tmp_path / "ber.json"
    assert ber.main(["--qc", "4,8,24,27,3,1", "--layered", "0.8125", "--layered-q8", "13",
                     "--crc", "CRC16:stop", "--ebn0", "3,30", "--frames", "64", "--iterations", "10",
                     "--precision", "1", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert "% CRC: frames passed / undetected errors / mean iterations" in text
    doc = json.loads(out.read_text())
    assert doc["crc"] == dict(name="CRC16", len=16, poly=0x1021, mode="stop")
    for name, r in doc["results"].items():
        print(name, r)
        assert len(r["crc_pass"]) == len(r["crc_undetected"]) == len(r["iters"]) == 2
        assert all(0 <= u <= p <= 64 for p, u in zip(r["crc_pass"], r["crc_undetected"]))
    for name in (ber.LAYERED, ber.LAYERED_Q8):
        r = doc["results"][name]
        assert r["crc_pass"][1] == 64 and r["crc_undetected"][1] == 0 and r["iters"][1] == 1.0
        assert r["ber"][1] == 0.0 and r["iters"][0] >= 1.0


def test_refusals_of_the_context_calls():
    import ldpc_ece535a as L
    c = code("B")
    dec = c.dec("circ", (0, 0, 0))
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*len must be in \[1, 24\] \(got 25\)"):
        dec.set_crc(25, 1)
    with pytest.raises(L.LdpcError, match=r"poly must be below 2\^len = 65536 \(got 65536\)"):
        dec.set_crc(16, 1 << 16)
    with pytest.raises(L.LdpcError, match="mode must be"):
        dec.set_crc(*cr.CRC16, mode="halt")
    small = code("E")                                  # K = 20
    with pytest.raises(L.LdpcError, match=r"A = K - filler = 20, len = 24"):
        small.dec().set_crc(*cr.CRC24A)
    dec.set_crc(*cr.CRC16)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*A = K - filler = 16, len = 16"):
        dec.set_rate_match(0, c.K - 16, 0)
    dec.set_rate_match(0, c.K - 17, 0)                 # A = len + 1 is legal
    dec.set_rate_match(0, 0, 0)
    dec.set_crc(0)
    dec.set_rate_match(0, c.K - 16, 0)                 # and with the CRC off, anything is
    dec.set_rate_match(0, 0, 0)
