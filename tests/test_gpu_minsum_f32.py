"""Min-sum at precision 1 (f32) on every route, against the float oracle.

f32 min-sum has no transcendental and no division: it is the reference's
decodeLogDomainSimple with `float` where the reference has `double`, and every
kernel is a template over Real.  So it has an exact contract -- the oracle's
float restatement (oracle.decode_batch(..., real="f32")), pinned on the CPU by
tests/test_minsum_f32_host.py -- and every assertion here is equality with it:
bits, packed bytes, iteration counts, syndrome weights and, where the route
returns them, posteriors as bit patterns.  No comparison leaves frames out.

The inputs are the sets of tests/minsum_f32_sets.py; the host tests show that
each of them separates float from double arithmetic and from a float
reference that sums a column in double or in another order.

The last section holds the methods whose arithmetic does not depend on the
precision mode (0, 2, 3 at precision 3; 2, 3 at precision 1) to the double
oracle on every shape case."""
import os

import numpy as np
import pytest

import ldpc_ece535a as L
import minsum_f32_sets as ms
import shape_cases as sc
from shape_cases import CAP, CASES, LARGE, SMALL, eq, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = L._capi.PREC_F32
KINDS = dict(launch={}, plain=dict(plain_layout=True), graph=dict(force_graph=True),
             onchip=dict(onchip=True))
PATHS = dict(plain=L._capi.PATH_SMALL, graph=L._capi.PATH_GRAPH, onchip=L._capi.PATH_ONCHIP)


def check(out, ref, what):
    eq(out, ref, what=what)
    same_bits(out["llr"], ref["post"], what=what)


def fits_onchip(H):
    M, N = H.shape
    return L._capi.plan_onchip(M, N, int(H.sum()), int(H.sum(1).max()), int(H.sum(0).max()),
                               method=0, precision=F32)["fits"]


class Routes:
    """The decoders of one dense H, one per route, made on first use."""

    def __init__(self, H, small):
        self.H, self.small, self._dec = np.array(H), small, {}

    def kinds(self):
        """launch, and for a code of the small-code kernel the plain layout
        and the forced large-code kernels; the on-chip kernels where they fit."""
        k = ["launch"] + (["plain", "graph"] if self.small else [])
        return k + (["onchip"] if fits_onchip(self.H) else [])

    def dec(self, kind):
        if kind not in self._dec:
            if self.small or kind != "launch":
                d = L.Decoder(self.H, reorder=False, **KINDS[kind])
            else:
                M, N = self.H.shape
                d = L.Decoder(csr=(M, N) + sc.dense_to_csr(self.H))
            want = PATHS.get(kind, L._capi.PATH_SMALL if self.small else L._capi.PATH_GRAPH)
            assert d.path == want, (kind, d.path)
            assert (d.H == self.H).all()
            self._dec[kind] = d
        return self._dec[kind]

    def schedules(self, kind):
        return (1, 2) if self.small and kind in ("launch", "plain") else (0,)

    def decode_all(self, s, what, kinds=None):
        """The set on every route (and both schedules of the small-code
        kernel), each equal to the float oracle."""
        ref = s.ref()
        for kind in kinds or self.kinds():
            d = self.dec(kind)
            for sched in self.schedules(kind):
                d.set_schedule(sched)
                out = d.decode(s.y, method=0, max_iters=s.cap, et_period=s.et, precision=F32,
                               polarity=s.polarity, want_llr=True)
                check(out, ref, "%s, %s route, schedule %d" % (what, kind, sched))
            d.set_schedule(0)

    def close(self):
        for d in self._dec.values():
            d.close()
        self._dec = {}


@pytest.fixture(scope="module")
def routes(request):
    c = CASES[request.param]
    r = Routes(c.H, c.small)
    yield r
    r.close()


@pytest.fixture(scope="module")
def default_routes():
    r = Routes(ms.default_h(), True)
    assert r.kinds() == ["launch", "plain", "graph", "onchip"]
    assert (L.Decoder().H == r.H).all()
    yield r
    r.close()


def cases(names):
    return pytest.mark.parametrize("routes", names, indirect=True)


# ---- a. every dispatch cell ----------------------------------------------------------------

@cases(SMALL + LARGE)
def test_dispatch_cells(routes, request):
    """Every shape case on its own launch path (both schedules and both
    layouts of the small-code kernel), every small case forced onto the
    large-code kernels, and every case the on-chip planner accepts there."""
    name = request.node.callspec.params["routes"]
    s = ms.get("shape/" + name)
    assert sc.early_and_capped(s.ref()["iters"]), name
    routes.decode_all(s, name)


@cases(list(ms.ET_CASES))
def test_et_period(routes, request):
    name = request.node.callspec.params["routes"]
    s = ms.get("shape/%s/et5" % name)
    assert (s.ref()["iters"] % 5 == 0).all()
    routes.decode_all(s, name + " et_period 5")


@cases(list(ms.SPECIAL))
def test_special_samples(routes, request):
    name = request.node.callspec.params["routes"]
    routes.decode_all(ms.get("special/" + name), name + " special samples")


# ---- b. the golden frames ---------------------------------------------------------------------

@pytest.mark.parametrize("cap", [5, 50])
@pytest.mark.parametrize("db", [0, 2, 4])
def test_default_h_fixture_frames(default_routes, db, cap):
    default_routes.decode_all(ms.get("default/db%d/cap%d" % (db, cap)),
                              "fixture frames %d dB cap %d" % (db, cap))


# ---- c. the persistent routes --------------------------------------------------------------------

def _persistent(name):
    """(decoder, set at et_period 1, set at et_period 5) of a code of
    tests/test_gpu_small_paths.py."""
    if name == ms.REFERENCE_H:
        return L.Decoder(), ms.get("persistent/reference_h/et1"), ms.get(
            "persistent/reference_h/et5")
    return (L.Decoder(np.array(CASES[name].H), reorder=False), ms.get("shape/" + name),
            ms.get("persistent/%s/et5" % name))


def _ring(dec, s, posts):
    """The set through one ring session, posted in batches of `posts` frames."""
    B = s.y.shape[0]
    assert sum(posts) == B
    d_y = torch.from_numpy(np.array(s.y)).cuda()
    pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
    it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    sy = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.ring_begin(method=0, max_iters=s.cap, et_period=s.et, precision=F32)
    lo, last = 0, None
    for n in posts:
        last = dec.ring_post(d_y.data_ptr() + 4 * dec.N * lo, n, pk.data_ptr() + dec.KB * lo,
                             it.data_ptr() + 4 * lo, sy.data_ptr() + 4 * lo)
        lo += n
    dec.ring_wait(last)
    dec.ring_end()
    torch.cuda.synchronize()
    return dict(packed=pk.cpu().numpy(), iters=it.cpu().numpy(), synd=sy.cpu().numpy())


@pytest.mark.parametrize("mode", [L._capi.MODE_LATENCY, L._capi.MODE_THROUGHPUT],
                         ids=["default", "throughput"])
@pytest.mark.parametrize("name", [ms.REFERENCE_H, "c_32x64"])
def test_ring_and_launch(name, mode):
    """The frame ring: three posted batches of 50, 77 and 65 frames, so the
    waves of a workgroup hold frames of two batches; et_period 1 and 5, on the
    ring and on the one-wave launch path at the same launch mode."""
    dec, s1, s5 = _persistent(name)
    dec.set_launch_mode(mode)
    dec.set_schedule(1)
    for s in (s1, s5):
        what = "%s et_period %d mode %d" % (name, s.et, mode)
        if s.et == 5:
            assert (s.ref()["iters"] % 5 == 0).all()
        out = dec.decode(s.y, method=0, max_iters=s.cap, et_period=s.et, precision=F32,
                         want_llr=True)
        check(out, s.ref(), what + ", launch")
        eq(_ring(dec, s, (50, 77, 65)), s.ref(), keys=("packed", "iters", "synd"),
           what=what + ", ring")
    dec.set_schedule(0)
    dec.set_launch_mode(L._capi.MODE_LATENCY)
    dec.close()


def _windows(s):
    """A span (37 stray samples, then 40 of the set's frames) and a round of
    300 windows: frame-aligned and arbitrary starts, both polarities; and the
    frames those windows hold."""
    N = s.csr[1]
    rng = np.random.Generator(np.random.PCG64(37))
    span = np.concatenate([rng.standard_normal(37).astype(np.float32), np.array(s.y[:40]).ravel()])
    p = rng.integers(0, span.size - N + 1, size=300).astype(np.int64)
    aligned = rng.random(300) < 0.5
    p[aligned] = 37 + N * rng.integers(0, 40, size=int(aligned.sum()))
    neg = rng.integers(0, 2, size=300).astype(np.int64)
    fr = np.stack([span[q:q + N] for q in p]).astype(np.float32)
    fr[neg == 1] = -fr[neg == 1]
    return span, (p << 1) | neg, fr


@pytest.mark.parametrize("name", [ms.REFERENCE_H, "c_32x64"])
def test_window_server_and_decode_windows(name):
    dec, s, _ = _persistent(name)
    span, win, fr = _windows(s)
    ref = ms.Set(name + " windows", fr, CAP, H=s.H).ref()
    assert sc.early_and_capped(ref["iters"])
    out = dec.decode_windows(span, win, method=0, max_iters=CAP, precision=F32)
    eq(out, ref, keys=("packed", "synd"), what=name + " decode_windows")
    dec.stage_span(span, max_windows=512)
    dec.serve_begin(method=0, max_iters=CAP, precision=F32, max_windows=512)
    got = [dec.serve_windows(w) for w in (win, win[:7], win[7:8])]
    dec.serve_end()
    eq(got[0], ref, keys=("packed", "synd"), what=name + " window server, round of 300")
    eq(got[1], {k: ref[k][:7] for k in ref}, keys=("packed", "synd"), what=name + " round of 7")
    eq(got[2], {k: ref[k][7:8] for k in ref}, keys=("packed", "synd"), what=name + " round of 1")
    dec.close()


# ---- d. the large-code pipeline and its knobs ---------------------------------------------------------

def _decoder(env=None, **kw):
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return L.Decoder(**kw)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _decode_set(d, s, what):
    out = d.decode(s.y, method=0, max_iters=s.cap, et_period=s.et, precision=F32, want_llr=True)
    check(out, s.ref(), what)
    return out


@pytest.mark.parametrize("env", [{}, {"LDPC_MSN_ORDER": "0"}, {"LDPC_MSN_ORDER": "1"},
                                 {"LDPC_MSN_CHUNKS": "5"}, {"LDPC_MSN_CHUNKS": "8"}],
                         ids=["default", "identity-order", "residue-order", "5-chunks", "8-chunks"])
def test_pipeline_knobs_dvbs2(env):
    """The DVB-S2-like code (N = 64800), 96 frames at 1.5 dB, cap 30: the
    narrow-chunk pipeline at its defaults, in either storage order and at 5
    and 8 chunks."""
    s = ms.get("dvb/knobs")
    assert sc.early_and_capped(s.ref()["iters"], 30)
    d = _decoder(env, csr=s.csr)
    assert d.pipeline()["chunks"] > 0
    _decode_set(d, s, "dvbs2_like %r" % (env,))
    d.close()


def test_post_kernels_info_first_order():
    """The information-first column order: the outputs come from the
    msn_post / msn_cols kernels."""
    s = ms.get("dvb/info_first")
    r = L._capi.plan_storage_order(s.csr)
    M, N = s.csr[:2]
    assert r["order"] == 1 and not np.array_equal(r["cpos"][M:], np.arange(M, N))
    d = _decoder(csr=s.csr)
    _decode_set(d, s, "dvbs2_like, information first")
    d.close()


@pytest.mark.parametrize("tag", list(ms.HIGH_DEGREE))
def test_high_check_degree(tag):
    """dc = 14 and dc = 20: the 16- and 32-slot check bodies and the
    degree-12 columns, at an Eb/N0 beyond the code's reach (every frame runs
    to the cap) and at one within it (every frame stops early)."""
    csr = ms.high_degree_code(*ms.HIGH_DEGREE[tag])
    assert int(np.diff(csr[2]).max()) == int(tag[2:])
    d = _decoder(csr=csr)
    assert d.pipeline()["chunks"] > 0
    hard, easy = ms.get(tag + "/3dB"), ms.get(tag + "/6dB")
    assert (hard.ref()["iters"] == hard.cap).all() and (easy.ref()["iters"] < easy.cap).all()
    _decode_set(d, hard, tag + " 3 dB")
    _decode_set(d, easy, tag + " 6 dB")
    d.close()


@pytest.fixture(scope="module")
def gdec():
    d = L.Decoder(force_graph=True)
    yield d
    d.close()


@pytest.mark.parametrize("et", [1, 5])
@pytest.mark.parametrize("B", ms.BATCHES)
def test_batches_recycle_every_slot(gdec, B, et):
    _decode_set(gdec, ms.get("batch/%d/et%d" % (B, et)), "B %d et_period %d" % (B, et))


# ---- e. where float and double part -------------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(ms.EDGES))
def test_edges(default_routes, tag):
    """+-inf and NaN samples; exact zeros of either sign; samples on a grid
    (tied minima, exactly-zero messages); amplitudes whose column sums
    overflow in float alone; amplitudes of 1e-30 and of 1e-40, which float
    holds as subnormals -- each on the small-code kernel, the large-code
    kernels and the on-chip kernels."""
    s = ms.get("edge/" + tag)
    post = s.ref()["post"]
    if tag == "overflow":
        assert np.isinf(post).any()
    if tag == "non_finite":
        assert np.isnan(post).any()
    if tag == "tiny":
        sub = np.abs(post[48:]) < np.finfo(np.float32).tiny
        assert (sub & (post[48:] != 0)).any()
    default_routes.decode_all(s, tag)


def test_degree_one_check_row():
    """A check of degree 1 sends the seed of its minimum, FLT_MAX, and the
    column sums built on it."""
    s = ms.get("edge/degree_one_row")
    assert (np.abs(s.ref()["post"]) >= np.finfo(np.float32).max / 2).any()
    r = Routes(s.H, True)
    assert r.kinds() == ["launch", "plain", "graph", "onchip"]
    r.decode_all(s, "degree-1 row")
    r.close()


# ---- f. methods whose arithmetic the precision mode does not change ----------------------------------------------

@pytest.mark.parametrize("method,prec", [(0, 3), (2, 3), (3, 3), (2, 1), (3, 1)])
@cases(SMALL + LARGE)
def test_precision_free_methods(routes, request, method, prec):
    """Min-sum, bit flipping and the hard decision at precision 3 are double
    arithmetic without a transcendental; bit flipping and the hard decision
    at precision 1 read the signs of the float samples only (their llr output
    is tx itself).  All equal the double oracle, posteriors included."""
    c = CASES[request.node.callspec.params["routes"]]
    ref = c.ref(method)
    d = routes.dec("launch")
    for sched in routes.schedules("launch"):
        d.set_schedule(sched)
        out = d.decode(c.frames, method=method, max_iters=CAP, precision=prec, want_llr=True)
        check(out, ref, "%s method %d precision %d schedule %d" % (c.name, method, prec, sched))
    d.set_schedule(0)
