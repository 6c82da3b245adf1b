"""Every kernel variant the shape dispatch picks, against the oracle.

tests/shape_cases.py holds one code per dispatch cell: the small-code
kernel's (NW, low / generic loops, column-centric or edge form, edge slots,
row slots) and the large-code kernels' degree bodies.  Each case is decoded
on the launch path (every method, both exact precisions, both schedules),
forced onto the large-code and on-chip kernels, through the device entry
point into guarded buffers, the frame ring and the window server, and
compared with the oracle's decode of the same frames: bits, packed bytes,
iteration counts, syndrome weights, and posteriors as bit patterns.  Of the
fast modes, min-sum is exact too (at f32 the oracle's float restatement, at
the compact f64 mode the oracle itself); fast sum-product, which has no
oracle, is held to what no rounding can change."""
import numpy as np
import pytest

import ldpc_ece535a as L
from shape_cases import B, CAP, CASES, LARGE, SMALL, early_and_capped, eq, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5


class Ctx:
    """A case and its decoders, one per path, made on first use."""

    def __init__(self, case):
        self.case = case
        self._dec = {}

    def dec(self, kind="launch"):
        if kind not in self._dec:
            c = self.case
            if c.small:
                kw = dict(launch={}, plain=dict(plain_layout=True), graph=dict(force_graph=True),
                          onchip=dict(onchip=True))[kind]
                d = L.Decoder(np.array(c.H), reorder=False, **kw)
            else:
                assert kind == "launch", kind
                d = L.Decoder(csr=c.csr)
            want = dict(launch=L._capi.PATH_SMALL if c.small else L._capi.PATH_GRAPH,
                        plain=L._capi.PATH_SMALL, graph=L._capi.PATH_GRAPH,
                        onchip=L._capi.PATH_ONCHIP)[kind]
            s = c.shape
            assert d.path == want, (c.name, kind, d.path)
            assert (d.M, d.N, d.E, d.KB, d.dc_max, d.dv_max) == (
                s["M"], s["N"], s["E"], s["KB"], s["dc"], s["dv"]), c.name
            assert (d.H == c.H).all(), c.name
            self._dec[kind] = d
        return self._dec[kind]

    def close(self):
        for d in self._dec.values():
            d.close()
        self._dec = {}


@pytest.fixture(scope="module")
def ctx(request):
    c = Ctx(CASES[request.param])
    yield c
    c.close()


def cases(names):
    return pytest.mark.parametrize("ctx", names, indirect=True)


def check(out, ref, what):
    eq(out, ref, what=what)
    same_bits(out["llr"], ref["post"], what=what)


def schedules(ctx, kind):
    return (1, 2) if ctx.case.small and kind in ("launch", "plain") else (0,)


# ---- 1. the launch path, exact modes -----------------------------------------------------

@pytest.mark.parametrize("method", [0, 1, 2, 3])
@cases(SMALL + LARGE)
def test_launch_exact(ctx, method):
    """The case's own path: methods 0-3, precisions 0 and 2, and on the
    small-code kernel both schedules (one wave / one workgroup per frame)."""
    c = ctx.case
    ref = c.ref(method)
    if method <= 2:
        assert early_and_capped(ref["iters"]), (c.name, method)
    dec = ctx.dec()
    for sched in schedules(ctx, "launch"):
        dec.set_schedule(sched)
        for prec in (0, 2):
            out = dec.decode(c.frames, method=method, max_iters=CAP, precision=prec, want_llr=True)
            check(out, ref, "%s method %d precision %d schedule %d" % (c.name, method, prec, sched))
    dec.set_schedule(0)


@pytest.mark.parametrize("method", [0, 1, 2, 3])
@cases(SMALL)
def test_small_cases_on_large_code_kernels(ctx, method):
    c = ctx.case
    dec = ctx.dec("graph")
    for prec in (0, 2):
        out = dec.decode(c.frames, method=method, max_iters=CAP, precision=prec, want_llr=True)
        check(out, c.ref(method), "%s forced to the large-code kernels, method %d precision %d" % (
            c.name, method, prec))


@pytest.mark.parametrize("method", [0, 1])
@cases(SMALL)
def test_small_cases_on_onchip_kernels(ctx, method):
    c = ctx.case
    dec = ctx.dec("onchip")
    for prec in (0, 2):
        out = dec.decode(c.frames, method=method, max_iters=CAP, precision=prec, want_llr=True)
        check(out, c.ref(method), "%s on the on-chip kernels, method %d precision %d" % (
            c.name, method, prec))


# ---- 2. et_period ---------------------------------------------------------------------------

@pytest.mark.parametrize("et", [1, 5])
@cases(["c_32x64", "g_250x256", "r_40x300"])
def test_et_period(ctx, et):
    c = ctx.case
    dec = ctx.dec()
    for method in (0, 1, 2):
        ref = c.ref(method, et=et)
        if et == 5:
            assert (ref["iters"] % 5 == 0).all()
        for sched in schedules(ctx, "launch"):
            dec.set_schedule(sched)
            out = dec.decode(c.frames, method=method, max_iters=CAP, et_period=et, want_llr=True)
            check(out, ref, "%s method %d et_period %d schedule %d" % (c.name, method, et, sched))
    dec.set_schedule(0)


# ---- 3. special samples -----------------------------------------------------------------------

def special_frames(c):
    """The case's frames with +-inf, NaN, +-0.0 and |y| = 45 samples on a
    stride of frames (the recipe of the non-finite tests)."""
    y = np.array(c.frames)
    y[::7, 3] = np.inf
    y[1::5, 10] = -np.inf
    y[2::9, 20] = np.nan
    y[3::4, 30:34] = 0.0
    y[5::8, 40:44] = -0.0
    y[6::11, 50] = 45.0
    y[7::13, 51] = -45.0
    return y


@pytest.mark.parametrize("method", [0, 1, 2, 3])
@cases(["c_32x64", "f_64x128", "s_48x96"])
def test_special_samples(ctx, method):
    c = ctx.case
    y = special_frames(c)
    ref = c.ref_for("special", method, y)
    dec = ctx.dec()
    for sched in schedules(ctx, "launch"):
        dec.set_schedule(sched)
        for prec in (0, 2):
            out = dec.decode(y, method=method, max_iters=CAP, precision=prec, want_llr=True)
            check(out, ref, "%s special samples, method %d precision %d schedule %d" % (
                c.name, method, prec, sched))
    dec.set_schedule(0)


# ---- 4. the device entry point, guarded outputs --------------------------------------------------

class Guarded:
    """A device output of `rows` rows, one row of guard bytes on each side."""

    def __init__(self, rows, width, dtype):
        self.t = torch.empty((rows + 2, width), dtype=dtype, device="cuda")
        self.t.view(torch.uint8).fill_(GUARD)
        self.row = width * self.t.element_size()
        self.ptr = self.t.data_ptr() + self.row

    def result(self, what):
        raw = self.t.cpu().numpy()
        edge = raw[[0, -1]].view(np.uint8)
        assert (edge == GUARD).all(), "%s: bytes outside the output were written" % what
        return raw[1:-1]


def guarded_outputs(dec, n, llr=True):
    o = dict(packed=Guarded(n, dec.KB, torch.uint8), bits=Guarded(n, dec.N, torch.uint8),
             iters=Guarded(n, 1, torch.int32), synd=Guarded(n, 1, torch.int32))
    if llr:
        o["llr"] = Guarded(n, dec.N, torch.float32)
    return o


def results(o, what):
    out = {k: g.result("%s %s" % (what, k)) for k, g in o.items()}
    for k in ("iters", "synd"):
        out[k] = out[k].reshape(-1)
    return out


@pytest.mark.parametrize("method", [0, 1])
@cases(["g_250x256", "b_48x64", "m_56x80", "e_24x64", "i_24x96", "r_40x300"])
def test_decode_device_guarded(ctx, method):
    """ldpc_decode_device into buffers one frame longer on each side: packed
    rows of 1, 2, 3, 5, 9 and 33 bytes, the last byte partial where K % 8 != 0."""
    c = ctx.case
    dec = ctx.dec()
    d_y = torch.from_numpy(np.array(c.frames)).cuda()
    o = guarded_outputs(dec, B)
    torch.cuda.synchronize()
    dec.decode_device(d_y.data_ptr(), B, o["packed"].ptr, method=method, max_iters=CAP,
                      d_bits=o["bits"].ptr, d_iters=o["iters"].ptr, d_synd=o["synd"].ptr,
                      d_llr=o["llr"].ptr)
    dec.synchronize()
    torch.cuda.synchronize()
    check(results(o, c.name), c.ref(method), "%s decode_device method %d" % (c.name, method))


# ---- 5. the frame ring ----------------------------------------------------------------------------

@pytest.mark.parametrize("method", [0, 1])
@cases(["c_32x64", "l_31x63", "k_37x101", "g_250x256"])
def test_ring(ctx, method):
    """Three batches of 64 frames posted in one session."""
    c = ctx.case
    dec = ctx.dec()
    d_y = torch.from_numpy(np.array(c.frames)).cuda()
    o = guarded_outputs(dec, B, llr=False)
    del o["bits"]
    torch.cuda.synchronize()
    dec.ring_begin(method=method, max_iters=CAP)
    ids = [dec.ring_post(d_y.data_ptr() + 4 * dec.N * lo, 64, o["packed"].ptr + dec.KB * lo,
                         o["iters"].ptr + 4 * lo, o["synd"].ptr + 4 * lo) for lo in (0, 64, 128)]
    dec.ring_wait(ids[-1])
    dec.ring_end()
    torch.cuda.synchronize()
    eq(results(o, c.name), c.ref(method), keys=("packed", "iters", "synd"),
       what="%s frame ring method %d" % (c.name, method))


# ---- 6. the window server -----------------------------------------------------------------------------

def span_and_rounds(c):
    """A span of 40 frames of the case's frames behind 37 stray samples, and
    rounds of 1, 7 and 300 windows: frame-aligned and arbitrary starts, both
    polarities."""
    N = c.H.shape[1]
    rng = np.random.Generator(np.random.PCG64(37))
    s = np.concatenate([rng.standard_normal(37).astype(np.float32), np.array(c.frames[:40]).ravel()])
    rounds = []
    for n in (1, 7, 300):
        p = rng.integers(0, s.size - N + 1, size=n).astype(np.int64)
        aligned = rng.random(n) < 0.5
        p[aligned] = 37 + N * rng.integers(0, 40, size=int(aligned.sum()))
        neg = rng.integers(0, 2, size=n).astype(np.int64)
        neg[aligned] &= rng.integers(0, 2, size=int(aligned.sum()))
        rounds.append((p << 1) | neg)
    return s, rounds


def window_ref(c, method, s, win, tag):
    N = c.H.shape[1]
    p, neg = win >> 1, (win & 1).astype(bool)
    fr = np.stack([s[q:q + N] for q in p]).astype(np.float32)
    fr[neg] = -fr[neg]
    return c.ref_for(tag, method, fr)


@pytest.mark.parametrize("method", [0, 1])
@cases(["b_48x64", "c_32x64", "d_8x32", "l_31x63", "m_56x80"])
def test_window_server(ctx, method):
    c = ctx.case
    dec = ctx.dec()
    s, rounds = span_and_rounds(c)
    dec.stage_span(s, max_windows=512)
    dec.serve_begin(method=method, max_iters=CAP, max_windows=512)
    got = [dec.serve_windows(w) for w in rounds]
    dec.serve_end()
    for i, (w, g) in enumerate(zip(rounds, got)):
        eq(g, window_ref(c, method, s, w, ("serve", i)), keys=("packed", "synd"),
           what="%s window server method %d, round of %d" % (c.name, method, w.size))


@cases(["g_250x256"])
def test_window_server_refuses_eight_slots(ctx):
    """KB = 1 fits the server's result granules, eight edge slots do not fit
    its workgroups: refused, and the context goes on decoding windows by
    launches."""
    c = ctx.case
    dec = ctx.dec()
    s, rounds = span_and_rounds(c)
    dec.stage_span(s, max_windows=512)
    with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED"):
        dec.serve_begin(method=1, max_iters=CAP, max_windows=512)
    w = rounds[2][:64]
    out = dec.decode_windows(s, w, method=1, max_iters=CAP)
    eq(out, window_ref(c, 1, s, w, "refused"), keys=("packed", "synd"),
       what="%s decode_windows after the refused serve_begin" % c.name)


# ---- 7. the fast modes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [1, 3])
@pytest.mark.parametrize("method", [0, 1])
@cases(SMALL + LARGE)
def test_fast_modes(ctx, method, prec):
    """Sum-product at precisions 1 (f32: ROCm's tanhf / logf) and 3 (compact
    f64: the device's reciprocal seed) has no host oracle: neither can be restated
    bit for bit on a host (on the default H, tests/test_gpu_sumproduct_inexact.py
    holds them to an oracle assembled from the device's functions).  On every
    shape, whatever the rounding: the noise-free frame
    decodes in one iteration to a zero syndrome and the oracle's bits (zero
    on every column that has a check), frames the oracle decodes within 5
    iterations get the oracle's decisions, and the planned and the plain
    layout give equal outputs bit for bit.  Min-sum has neither function: at
    precision 1 it is the reference's arithmetic in float and equals the
    oracle's float restatement on all frames, at precision 3 it is double
    arithmetic and equals the oracle itself, posteriors as bit patterns
    included."""
    c = ctx.case
    dec = ctx.dec()
    N = c.H.shape[1]
    clean = -np.ones((3, N), np.float32)
    cref = c.ref_for("clean", method, clean)
    assert (cref["bits"][:, c.H.sum(0) > 0] == 0).all() and (cref["synd"] == 0).all()
    ref = c.ref(method)
    easy = ref["iters"] <= 5
    assert easy.any(), c.name
    for sched in schedules(ctx, "launch"):
        dec.set_schedule(sched)
        what = "%s method %d precision %d schedule %d" % (c.name, method, prec, sched)
        out = dec.decode(clean, method=method, max_iters=CAP, precision=prec)
        eq(out, cref, keys=("bits", "packed", "synd"), what=what + ", noise-free")
        assert (out["iters"] <= 1).all(), what
        out = dec.decode(c.frames, method=method, max_iters=CAP, precision=prec, want_llr=True)
        np.testing.assert_array_equal(out["bits"][easy], ref["bits"][easy], err_msg=what)
        np.testing.assert_array_equal(out["packed"][easy], ref["packed"][easy], err_msg=what)
        if method == 0:
            check(out, c.ref_f32() if prec == 1 else ref, what + ", all frames")
        if c.small:
            plain = ctx.dec("plain")
            plain.set_schedule(sched)
            other = plain.decode(c.frames, method=method, max_iters=CAP, precision=prec,
                                 want_llr=True)
            plain.set_schedule(0)
            eq(out, other, what=what + ", planned vs plain layout")
            same_bits(out["llr"], other["llr"], what=what + ", planned vs plain layout")
    dec.set_schedule(0)
