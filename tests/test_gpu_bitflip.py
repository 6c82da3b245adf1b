"""Bit flipping on codes where a bit really flips, against the oracle.

On every other code of the suite no column has more than M / 2 checks, the
vote of decodeBitFlipping (lib/ldpc_decoder_cb_impl.cc:455-467) never
succeeds and method 2 is method 3 with an iteration count.  The codes of
tests/bitflip_cases.py have such columns; tests/test_bitflip_ref_host.py
holds the oracle to the reference's text on them and shows that their frames
flip, keep changing after iteration 1, stop at 1, in between and at the cap
(within one 64-frame chunk), and tell a wrong vote from the right one.  Here
the kernels decode the same frames: decode_frame's METHOD == 2 branch for
NW 1 and 4 (csrc/ldpc_frame.hpp) and g_check_bf / g_var_bf<4 / 8 / 16> /
g_decide (csrc/ldpc_graph.hip), on every route to them.  Everything is
integer arithmetic at every precision: bits, packed bytes, iteration counts
and syndrome weights equal the oracle's, posteriors (the samples) as bit
patterns."""
import numpy as np
import pytest

import ldpc_ece535a as L
from bitflip_cases import CASES, FRAMES, LARGE, NO_LATER, SMALL, early_mid_capped
from shape_cases import CAP, eq, same_bits, threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
CAPS = (1, 2, 20)
PRECS = (0, 1, 2, 3)


class Ctx:
    """A case and its decoders, one per route, made on first use.  launch:
    the case's own path; plain: the small-code kernel on the CSR-order
    layout; graph, csr_graph: a small case forced onto the large-code kernels
    (g_var_bf<4>), from the dense H and from CSR; onchip: an on-chip context,
    which has no bit-flip kernel of its own and runs the large-code ones."""

    def __init__(self, case):
        self.case = case
        self._dec = {}

    def dec(self, kind="launch"):
        if kind not in self._dec:
            c = self.case
            if kind == "csr_graph" or not c.small:
                assert kind in ("launch", "csr_graph"), kind
                d = L.Decoder(csr=c.csr, force_graph=kind == "csr_graph")
            else:
                kw = dict(launch={}, plain=dict(plain_layout=True), graph=dict(force_graph=True),
                          onchip=dict(onchip=True))[kind]
                d = L.Decoder(np.array(c.H), reorder=False, **kw)
            small = c.small and kind in ("launch", "plain")
            want = (L._capi.PATH_SMALL if small else L._capi.PATH_ONCHIP if kind == "onchip"
                    else L._capi.PATH_GRAPH)
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


def routes(ctx):
    """(kind, schedule) of every launch a case's own path has."""
    if ctx.case.small:
        return [(k, s) for k in ("launch", "plain") for s in (1, 2)]
    return [("launch", 0)]


def run(ctx, kind, sched, y, **kw):
    dec = ctx.dec(kind)
    if sched:
        dec.set_schedule(sched)
    try:
        return dec.decode(y, method=kw.pop("method", 2), want_llr=True, **kw)
    finally:
        if sched:
            dec.set_schedule(0)


# ---- 1. every case on its own path -----------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
@cases(SMALL + LARGE)
def test_own_path(ctx, cap):
    """Caps 1, 2 and 20, precisions 0-3; the small cases with the planned and
    the plain layout under both schedules.  At the cap of 20 the frames hold
    every kind of stop, at 2 a flip of iteration 2 is the last thing done."""
    c = ctx.case
    ref = c.ref(2, cap)
    if cap == CAP:
        assert (ref["bits"] != c.ref(3)["bits"]).any(), c.name
        if c.name not in NO_LATER:
            assert (ref["bits"] != c.ref(2, 1)["bits"]).any(), c.name
        if c.found:
            assert early_mid_capped(ref["iters"][:64]), c.name
    for kind, sched in routes(ctx):
        for prec in PRECS:
            out = run(ctx, kind, sched, c.frames, max_iters=cap, precision=prec)
            check(out, ref, "%s %s cap %d precision %d schedule %d" % (c.name, kind, cap, prec, sched))


# ---- 2. the small cases on the large-code kernels: g_var_bf<4> ---------------------------------

@pytest.mark.parametrize("kind", ["graph", "csr_graph"])
@cases(SMALL)
def test_small_cases_on_large_code_kernels(ctx, kind):
    c = ctx.case
    assert ctx.dec(kind).dv_max <= 4
    for cap in CAPS:
        for prec in PRECS:
            out = run(ctx, kind, 0, c.frames, max_iters=cap, precision=prec)
            check(out, c.ref(2, cap), "%s %s cap %d precision %d" % (c.name, kind, cap, prec))


@cases(["a_5x14"])
def test_onchip_context_runs_the_large_code_kernels(ctx):
    """The on-chip planner accepts a code this small; its context decodes
    methods 2 and 3 on the large-code kernels."""
    c = ctx.case
    s = c.shape
    assert L._capi.plan_onchip(s["M"], s["N"], s["E"], s["dc"], s["dv"])["fits"]
    for cap in CAPS:
        out = run(ctx, "onchip", 0, c.frames, max_iters=cap)
        check(out, c.ref(2, cap), "%s on-chip context cap %d" % (c.name, cap))
    check(run(ctx, "onchip", 0, c.frames, method=3, max_iters=CAP), c.ref(3),
          "%s on-chip context method 3" % c.name)


# ---- 3. et_period ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ctx,kind", [("a_5x14", "launch"), ("c_5x70", "launch"), ("c_5x70", "graph"),
                                      ("e_11x40", "launch"), ("h_20x40", "launch")],
                         indirect=["ctx"])
def test_et_period(ctx, kind):
    """The exit test every 5th iteration only: every count a multiple of 5,
    some frame later than at et_period 1; NW 1 and 4 and bodies 4, 8, 16."""
    c = ctx.case
    ref = c.ref(2, et=5)
    assert (ref["iters"] % 5 == 0).all() and (ref["iters"] > c.ref(2)["iters"]).any()
    for k, sched in (routes(ctx) if kind == "launch" else [(kind, 0)]):
        out = run(ctx, k, sched, c.frames, max_iters=CAP, et_period=5)
        check(out, ref, "%s %s et_period 5 schedule %d" % (c.name, k, sched))
        assert (out["iters"] % 5 == 0).all()
    # a cap that is no multiple of the period: the last tested iteration is 5
    ref = c.ref(2, 7, et=5)
    assert set(np.unique(ref["iters"])) <= {5, 7}
    check(run(ctx, kind, 0, c.frames, max_iters=7, et_period=5), ref, "%s cap 7 et_period 5" % c.name)


# ---- 4. polarity and the other entry points ----------------------------------------------------------

def oracle(c, y, cap=CAP, polarity=1.0, method=2):
    from oracle import oracle as orc
    return orc.decode_batch(method, c.H, y, cap, polarity=polarity, nthreads=threads(), want_post=True)


class Guarded:
    """A device output of `rows` rows, one row of guard bytes on each side."""

    def __init__(self, rows, width, dtype):
        self.t = torch.empty((rows + 2, width), dtype=dtype, device="cuda")
        self.t.view(torch.uint8).fill_(GUARD)
        self.ptr = self.t.data_ptr() + width * self.t.element_size()

    def result(self, what):
        raw = self.t.cpu().numpy()
        assert (raw[[0, -1]].view(np.uint8) == GUARD).all(), "%s: bytes outside the output were written" % what
        return raw[1:-1]


ENTRY = ["a_5x14", "c_5x70", "e_11x40", "h_20x40"]


@cases(ENTRY)
def test_opposite_polarity(ctx):
    """Polarity -1 complements y, so other columns flip: the oracle on the
    negated samples, and not the complement of the polarity +1 result."""
    c = ctx.case
    ref = oracle(c, c.frames, polarity=-1.0)
    eq(ref, oracle(c, -np.array(c.frames)), what=c.name)
    assert (ref["bits"] != oracle(c, c.frames, polarity=-1.0, method=3)["bits"]).any(), c.name
    assert (ref["bits"] != 1 - c.ref(2)["bits"]).any(), c.name
    for kind, sched in routes(ctx) + ([("graph", 0)] if c.small else []):
        out = run(ctx, kind, sched, c.frames, max_iters=CAP, polarity=-1.0)
        check(out, ref, "%s %s polarity -1 schedule %d" % (c.name, kind, sched))


@cases(ENTRY)
def test_decode_both(ctx):
    """Both polarities of interleaved samples at once: one launch on the
    small path (pm_half), one per polarity on the large one."""
    c = ctx.case
    z = np.zeros(2 * c.frames.size + 3, np.float32)
    z[3::2] = c.frames.ravel()
    z[4::2] = 9.0     # the imaginary parts are not read
    ref = {p: oracle(c, c.frames, polarity=p) for p in (1.0, -1.0)}
    for kind in ("launch",) + (("graph",) if c.small else ()):
        for cap, want in ((CAP, ref), (2, {p: oracle(c, c.frames, 2, polarity=p) for p in (1.0, -1.0)})):
            both = ctx.dec(kind).decode_both(z[3:], method=2, max_iters=cap, cw_stride=2 * c.H.shape[1],
                                             elem_stride=2, B=FRAMES)
            for half, p in ((0, 1.0), (1, -1.0)):
                got = {k: both[k][half * FRAMES:(half + 1) * FRAMES] for k in ("packed", "synd")}
                eq(got, want[p], keys=("packed", "synd"),
                   what="%s %s decode_both cap %d polarity %+d" % (c.name, kind, cap, p))


@cases(ENTRY)
def test_decode_windows(ctx):
    """Windows at frame starts and at arbitrary positions of one span, either
    polarity: the oracle on the same samples."""
    c = ctx.case
    N = c.H.shape[1]
    rng = np.random.Generator(np.random.PCG64(37))
    s = np.concatenate([rng.standard_normal(37).astype(np.float32), np.array(c.frames[:64]).ravel()])
    pos = np.concatenate([37 + N * np.arange(64), rng.integers(0, s.size - N + 1, size=70)])
    neg = np.concatenate([np.zeros(64, np.int64), rng.integers(0, 2, size=70), ])
    neg[32:64] = 1
    win = (pos.astype(np.int64) << 1) | neg
    fr = np.stack([s[p:p + N] for p in pos]).astype(np.float32)
    fr[neg == 1] = -fr[neg == 1]
    ref = oracle(c, fr)
    eq({k: ref[k][:32] for k in ("packed", "synd")}, {k: c.ref(2)[k][:32] for k in ("packed", "synd")},
       keys=("packed", "synd"), what=c.name)
    assert (ref["bits"] != oracle(c, fr, method=3)["bits"]).any()
    for kind in ("launch",) + (("graph",) if c.small else ()):
        out = ctx.dec(kind).decode_windows(s, win, method=2, max_iters=CAP)
        eq(out, ref, keys=("packed", "synd"), what="%s %s decode_windows" % (c.name, kind))


@cases(ENTRY)
def test_decode_device_guarded(ctx):
    """ldpc_decode_device into buffers one frame longer on each side."""
    c = ctx.case
    dec = ctx.dec()
    d_y = torch.from_numpy(np.array(c.frames)).cuda()
    o = dict(packed=Guarded(FRAMES, dec.KB, torch.uint8), bits=Guarded(FRAMES, dec.N, torch.uint8),
             iters=Guarded(FRAMES, 1, torch.int32), synd=Guarded(FRAMES, 1, torch.int32),
             llr=Guarded(FRAMES, dec.N, torch.float32))
    torch.cuda.synchronize()
    dec.decode_device(d_y.data_ptr(), FRAMES, o["packed"].ptr, method=2, max_iters=CAP,
                      d_bits=o["bits"].ptr, d_iters=o["iters"].ptr, d_synd=o["synd"].ptr,
                      d_llr=o["llr"].ptr)
    dec.synchronize()
    torch.cuda.synchronize()
    out = {k: g.result("%s %s" % (c.name, k)) for k, g in o.items()}
    for k in ("iters", "synd"):
        out[k] = out[k].reshape(-1)
    check(out, c.ref(2), "%s decode_device" % c.name)


# ---- 5. special samples ------------------------------------------------------------------------------------

@cases(["a_5x14", "c_5x70", "g_31x62"])
def test_special_samples(ctx):
    """+-0.0, NaN and +-inf at columns that can flip: y = !(rx < 0), so the
    zeros and NaN decide 1 under either polarity."""
    c = ctx.case
    y = c.special_frames()
    for pol in (1.0, -1.0):
        ref = oracle(c, y, polarity=pol)
        assert (ref["bits"] != oracle(c, y, polarity=pol, method=3)["bits"]).any()
        for kind, sched in routes(ctx) + ([("graph", 0)] if c.small else []):
            for prec in (0, 1):
                out = run(ctx, kind, sched, y, max_iters=CAP, precision=prec, polarity=pol)
                what = "%s %s special samples, polarity %+d precision %d schedule %d" % (
                    c.name, kind, pol, prec, sched)
                eq(out, ref, what=what)
                if pol > 0:
                    same_bits(out["llr"], ref["post"], what=what)
                else:   # NaN * -1: the sign of the product's NaN is the multiplier's business
                    np.testing.assert_array_equal(out["llr"], ref["post"], err_msg=what)


# ---- 6. the control ----------------------------------------------------------------------------------------

@cases(SMALL + LARGE)
def test_method_3_is_the_control(ctx):
    """The hard decision of the same frames equals the oracle's and differs
    from method 2's: what the tests above compare is the vote."""
    c = ctx.case
    ref3 = c.ref(3)
    assert (ref3["bits"] != c.ref(2)["bits"]).any() and (ref3["packed"] != c.ref(2)["packed"]).any()
    assert (ref3["iters"] == 0).all()
    for kind, sched in routes(ctx) + ([("graph", 0)] if c.small else []):
        out = run(ctx, kind, sched, c.frames, method=3, max_iters=CAP)
        check(out, ref3, "%s %s method 3 schedule %d" % (c.name, kind, sched))
