"""Sum-product at precisions 1 (f32) and 3 (f64 fast) against an oracle
assembled from the device's own functions.

A host cannot restate ROCm's tanhf / logf or the compact double forms that
start from the device's reciprocal seed, but it only has to evaluate them:
everything else in sum-product is single IEEE operations.  The reference here
is tests/sumproduct_ref.py -- numpy, held to the C oracle bit for bit on the
host -- with tanh_half and check_msg evaluated elementwise on the device by
ldpc_math_probe.  Every route whose kernels make scalar Math<PREC> calls must
equal it exactly: bits, packed bytes, iterations, syndrome weights and
posteriors as bit patterns (NaN positions equal), at caps 1, 5 and 50 and
et_period 1 and 5, on 64 ordinary frames (some stop early, some reach the
cap), 32 frames far outside the channel's range and 16 with +-inf / NaN
samples.  tests/test_gpu_math.py holds the two functions themselves.

The small-code route at precision 3 picks batched and single-range forms per
frame, so it has no elementwise restatement: at cap 1 its posteriors must lie
in the enclosure of sumproduct_ref.enclosure_cap1."""
import numpy as np
import pytest

import ldpc_ece535a as L
import shape_cases as sc
import sumproduct_ref as spr
import sumproduct_sets as ss
from oracle import oracle as orc
from math_probe import Probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C = L._capi
PRECS = (C.PREC_F32, C.PREC_F64_FAST)
LARGE_CASE = "u_48x96"   # the smallest large-code case
_refs = {}


@pytest.fixture(scope="module")
def probe():
    p = Probe()
    yield p
    p.close()


def frames():
    """the 112 frames, one batch: ordinary 0..63, extreme 64..95, non-finite 96..111"""
    if "y" not in _refs:
        y = np.concatenate([ss.ordinary(), ss.extreme(), ss.nonfinite()])
        y.setflags(write=False)
        _refs["y"] = y
    return _refs["y"]


def device_fns(probe, prec):
    real = np.float32 if prec == C.PREC_F32 else np.float64

    def fn(which):
        return lambda x: probe(which, prec, x).reshape(x.shape)
    return dict(tanh_half=fn(C.PROBE_TANH_HALF), check_msg=fn(C.PROBE_CHECK_MSG), Real=real)


def ref(probe, prec, cap, et, key="default"):
    """the assembled oracle's result, computed once per cell and left unchanged"""
    k = (key, prec, cap, et)
    if k not in _refs:
        if key == "default":
            csr, y = ss.default_csr(), frames()
        else:
            c = sc.CASES[key]
            csr, y = c.csr, c.frames[:16]
        r = spr.decode(csr, y, cap, et_period=et, **device_fns(probe, prec))
        for v in r.values():
            v.setflags(write=False)
        _refs[k] = r
    return _refs[k]


def host_decode(dec, y, prec, cap, et):
    out = dec.decode(y, method=1, max_iters=cap, et_period=et, precision=prec, want_llr=True)
    out["post"] = out.pop("llr")
    return out


def device_decode(dec, y, prec, cap, et):
    n, N = y.shape
    d_y = torch.from_numpy(np.array(y)).cuda()
    pk = torch.zeros((n, dec.KB), dtype=torch.uint8, device="cuda")
    bt = torch.zeros((n, N), dtype=torch.uint8, device="cuda")
    it = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sy = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ll = torch.zeros((n, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_device(d_y.data_ptr(), n, pk.data_ptr(), method=1, max_iters=cap, et_period=et,
                      precision=prec, d_bits=bt.data_ptr(), d_iters=it.data_ptr(),
                      d_synd=sy.data_ptr(), d_llr=ll.data_ptr())
    dec.synchronize()
    return dict(packed=pk.cpu().numpy(), bits=bt.cpu().numpy(), iters=it.cpu().numpy(),
                synd=sy.cpu().numpy(), post=ll.cpu().numpy())


def ring_decode(dec, y, prec, cap, et):
    """one ring session of two posted batches"""
    n, N = y.shape
    d_y = torch.from_numpy(np.array(y)).cuda()
    pk = torch.zeros((n, dec.KB), dtype=torch.uint8, device="cuda")
    it = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sy = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.ring_begin(method=1, max_iters=cap, et_period=et, precision=prec)
    half = n // 2
    ids = [dec.ring_post(d_y.data_ptr() + 4 * N * lo, hi - lo, pk.data_ptr() + dec.KB * lo,
                         it.data_ptr() + 4 * lo, sy.data_ptr() + 4 * lo)
           for lo, hi in ((0, half), (half, n))]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    return dict(packed=pk.cpu().numpy(), iters=it.cpu().numpy(), synd=sy.cpu().numpy())


@pytest.fixture(scope="module")
def decoders():
    d = dict(graph=L.Decoder(force_graph=True), onchip=L.Decoder(onchip=True), small=L.Decoder())
    assert d["graph"].path == C.PATH_GRAPH and d["onchip"].path == C.PATH_ONCHIP
    assert d["small"].path == C.PATH_SMALL
    for dec in d.values():
        assert (dec.H == ss.default_h()).all()
    yield d
    for dec in d.values():
        dec.close()


def test_the_oracle_distinguishes_the_precisions(probe):
    """the assembled oracle of precision 1 is float arithmetic: its posteriors
    differ from the double oracle's and from precision 3's on every frame"""
    y = frames()[:64]
    it50 = orc.decode_batch(1, ss.default_h(), y, 50)["iters"]   # by the C oracle alone
    assert (it50 < 50).sum() >= 16 and (it50 == 50).sum() >= 4
    f64 = orc.decode_batch(1, ss.default_h(), frames(), 5, want_post=True)["post"][:64]
    p1 = ref(probe, C.PREC_F32, 5, 1)["post"][:64]
    p3 = ref(probe, C.PREC_F64_FAST, 5, 1)["post"][:64]
    assert y.shape[0] == 64
    assert (~ss.same_posteriors(p1, f64)).any(axis=1).all()
    assert (~ss.same_posteriors(p1, p3)).any(axis=1).all()


CELLS = [(cap, et) for cap in ss.CAPS for et in ss.ETS]


@pytest.mark.parametrize("cap,et", CELLS)
@pytest.mark.parametrize("prec", PRECS)
def test_large_code_and_onchip_kernels(probe, decoders, prec, cap, et):
    """Decoder(force_graph=True) and Decoder(onchip=True) on the default H"""
    r = ref(probe, prec, cap, et)
    for kind in ("graph", "onchip"):
        out = host_decode(decoders[kind], frames(), prec, cap, et)
        ss.assert_same(out, r, "%s precision %d cap %d et_period %d" % (kind, prec, cap, et))


@pytest.mark.parametrize("cap,et", CELLS)
@pytest.mark.parametrize("prec", PRECS)
def test_decode_device_in_both_launch_modes(probe, decoders, prec, cap, et):
    """decode_device at either launch mode: on the large-code and on-chip
    kernels, and at precision 1 on the small-code kernel too"""
    r = ref(probe, prec, cap, et)
    kinds = ("graph", "onchip") + (("small",) if prec == C.PREC_F32 else ())
    for kind in kinds:
        dec = decoders[kind]
        try:
            for mode in (C.MODE_LATENCY, C.MODE_THROUGHPUT):
                dec.set_launch_mode(mode)
                out = device_decode(dec, frames(), prec, cap, et)
                ss.assert_same(out, r, "decode_device %s mode %d precision %d cap %d et_period %d"
                               % (kind, mode, prec, cap, et))
        finally:
            dec.set_launch_mode(C.MODE_LATENCY)


@pytest.mark.parametrize("cap,et", CELLS)
def test_f32_small_code_route(probe, decoders, cap, et):
    """Math<1> is scalar calls on every route: the small-code kernel at both
    schedules, and a ring session of two posted batches"""
    prec = C.PREC_F32
    r = ref(probe, prec, cap, et)
    dec = decoders["small"]
    try:
        for sched in (1, 2):
            dec.set_schedule(sched)
            out = host_decode(dec, frames(), prec, cap, et)
            ss.assert_same(out, r, "small-code schedule %d cap %d et_period %d" % (sched, cap, et))
        dec.set_schedule(1)
        out = ring_decode(dec, frames(), prec, cap, et)
        ss.assert_same(out, r, "ring cap %d et_period %d" % (cap, et))
    finally:
        dec.set_schedule(0)


@pytest.mark.parametrize("prec", PRECS)
def test_a_larger_code(probe, prec):
    """the smallest large-code shape case on the large-code path: 16 frames, cap 10"""
    c = sc.CASES[LARGE_CASE]
    dec = L.Decoder(csr=c.csr)
    assert dec.path == C.PATH_GRAPH
    r = ref(probe, prec, 10, 1, key=LARGE_CASE)
    assert sc.early_and_capped(orc.decode_batch(1, c.H, c.frames[:16], 10)["iters"], 10)
    out = host_decode(dec, c.frames[:16], prec, 10, 1)
    ss.assert_same(out, r, "%s precision %d" % (LARGE_CASE, prec))
    dec.close()


@pytest.mark.parametrize("name", ["ordinary", "scaled by 8"])
def test_fast_small_code_route_in_the_enclosure(decoders, name):
    """Precision 3 on the small-code kernel at cap 1, both schedules: every
    posterior inside the enclosure, every decision the enclosure fixes.  The
    ordinary frames keep every |m| <= LDPC_TANH_SPLIT = 16 (the batched open
    log runs); each frame scaled by 8 holds a sample beyond it (the two-range
    tanh's frame: the saturating table log runs)."""
    y = ss.ordinary() if name == "ordinary" else ss.extreme()[:8]
    if name == "ordinary":
        assert (np.abs(y) <= 16.0).all()
    else:
        assert (np.abs(y) > 16.0).any(axis=1).all()
    lo, hi = spr.enclosure_cap1(ss.default_csr(), y, orc.tanh_half)
    dec = decoders["small"]
    try:
        for sched in (1, 2):
            dec.set_schedule(sched)
            out = dec.decode(y, method=1, max_iters=1, precision=C.PREC_F64_FAST, want_llr=True)
            fixed = spr.assert_enclosed(out, lo, hi, "%s frames, schedule %d" % (name, sched))
            assert fixed > 0.9   # the enclosure decides nearly every bit
            assert (out["iters"] == 1).all()
    finally:
        dec.set_schedule(0)
