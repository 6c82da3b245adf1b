"""The inputs of the f32 min-sum parity tests, shared by the host tests
(tests/test_minsum_f32_host.py: every set separates float from double
arithmetic and from two mutated float references) and the GPU tests
(tests/test_gpu_minsum_f32.py and the f32 legs of the older files: every route
equals the float oracle on them).

A set is a code, frames, an iteration cap and an et_period.  SETS maps a
name to a function that builds it; get(name) builds it once per process, and
Set.ref() / Set.ref64() are the float and the double oracle's results on it
(posteriors included), computed once."""
import os

import numpy as np

import shape_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = sc.KEYS


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


class Set:
    def __init__(self, name, y, cap, et=1, H=None, csr=None, polarity=1.0):
        self.name, self.cap, self.et, self.polarity = name, cap, et, polarity
        if csr is None:
            H = np.ascontiguousarray(H, np.uint8)
            rp, ci = sc.dense_to_csr(H)
            csr = (H.shape[0], H.shape[1], rp, ci)
        self.H, self.csr = H, csr
        self.y = np.ascontiguousarray(y, np.float32)
        self.y.setflags(write=False)
        self._ref = {}

    @property
    def dv_max(self):
        return int(np.bincount(self.csr[3], minlength=self.csr[1]).max())

    def _oracle(self, real):
        from oracle import oracle as orc
        M, N, rp, ci = self.csr
        kw = dict(nthreads=sc.threads(), et_period=self.et, polarity=self.polarity)
        if real == "f32":
            return orc.decode_batch_sparse(0, rp, ci, M, N, self.y, self.cap, real="f32",
                                           want_post=True, **kw)
        if self.H is not None:
            return orc.decode_batch(0, self.H, self.y, self.cap, want_post=True, **kw)
        return orc.decode_batch_sparse(0, rp, ci, M, N, self.y, self.cap, **kw)

    def head(self, n):
        """The set's first n frames as a set of their own."""
        return Set("%s[:%d]" % (self.name, n), self.y[:n], self.cap, et=self.et, H=self.H,
                   csr=self.csr, polarity=self.polarity)

    def ref(self):
        """The float oracle's bits, packed, iters, synd and post."""
        if "f32" not in self._ref:
            self._ref["f32"] = self._oracle("f32")
        return self._ref["f32"]

    def ref64(self):
        """The double oracle's; post (cast to float) only where the set holds a
        dense H (the sparse double oracle returns none)."""
        if "f64" not in self._ref:
            self._ref["f64"] = self._oracle("f64")
        return self._ref["f64"]


# ---- frames -------------------------------------------------------------------------

def default_h():
    return golden("frames_default.npz")["H_reordered"]


def non_finite_frames():
    """The frames of test_gpu_decode.py::test_non_finite_samples."""
    y = golden("frames_default.npz")["db2_llr"].copy()
    rng = np.random.default_rng(99)
    for b in range(0, y.shape[0], 3):  # every third frame gets 1-3 bad samples
        for _ in range(1 + b % 3):
            y[b, rng.integers(0, 64)] = rng.choice([np.inf, -np.inf, np.nan])
    return y


def zero_frames():
    """Exact zeros of either sign: whole frames, every other sample, runs."""
    y = golden("frames_default.npz")["db2_llr"].copy()
    y[3::4, 30:34] = 0.0
    y[5::8, 40:44] = -0.0
    y[0] = 0.0
    y[1] = -0.0
    y[2, ::2] = 0.0
    y[6, 1::2] = -0.0
    return y


def quantised_frames():
    """Multiples of 0.25 (48 frames: many tied minima and exactly-zero
    messages, and every sum exact in either type), then the same multiples
    times float32(0.1) (48 frames: the same ties, but sums that round)."""
    q = np.round(golden("frames_default.npz")["db0_llr"].astype(np.float64) * 4) / 4
    y = q.astype(np.float32)
    y[48:] = y[48:] * np.float32(0.1)
    return y


def overflow_frames():
    """|y| in [1e37, 3e38], log-uniform by the rank of the 0 dB fixture's
    amplitudes: column sums overflow in float and not in double."""
    y = golden("frames_default.npz")["db0_llr"].astype(np.float64)
    rank = np.argsort(np.argsort(np.abs(y), axis=None)).reshape(y.shape) / (y.size - 1.0)
    out = (np.sign(y) * 1e37 * 30.0 ** rank).astype(np.float32)
    assert np.isfinite(out).all() and np.abs(out).min() >= 1e37 and np.abs(out).max() <= 3e38
    return out


def tiny_frames():
    """Amplitudes of 1e-30 (normal) and 1e-40 (subnormal in float)."""
    base = golden("frames_default.npz")["db2_llr"].astype(np.float64)
    y = np.concatenate([base[:48] * 1e-30, base[:48] * 1e-40]).astype(np.float32)
    assert (np.abs(y[48:]) < np.finfo(np.float32).tiny).all() and (y[48:] != 0).any()
    return y


def degree_one_row_code():
    """e_24x64 with row 0 cut down to column 7 alone (a check of degree 1: its
    message is the minimum's seed, +-FLT_MAX) and row 1 to columns 7 and 9."""
    H = np.array(sc.CASES["e_24x64"].H)
    H[0, :] = 0
    H[0, 7] = 1
    H[1, :] = 0
    H[1, [7, 9]] = 1
    assert H.sum(1).min() == 1
    return H


def mixed_frames(H, B, seed, dbs=(0, 1, 2, 3, 4)):
    """Random codewords of a dense H at a mix of Eb/N0 (encoded on the host)."""
    import ldpc_ece535a as L
    rng = np.random.default_rng(seed)
    M, N = H.shape
    x = 2.0 * L.encode(H, rng.integers(0, 2, size=(B, N - M), dtype=np.uint8)) - 1.0
    db = rng.choice(np.asarray(dbs, np.float64), size=B)
    return (x + np.sqrt(10.0 ** (-db / 10.0))[:, None] * rng.standard_normal(x.shape)).astype(
        np.float32)


def ira_noisy(csr, B, seed, db):
    from ldpc_ece535a import codes
    M, N = csr[0], csr[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, N - M), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


def dvb_code():
    from ldpc_ece535a import codes
    return codes.dvbs2_like(0)


def dvb_info_first():
    """(csr2, permute): the DVB-S2-like code with its columns in the ETSI
    order, and the map of parity-first frames onto it
    (test_gpu_ms_paths.py::test_post_kernels_info_first_order)."""
    M, N, rp, ci = dvb_code()
    K = N - M
    newcol = np.where(ci >= M, ci - M, ci + K).astype(np.int64)
    rows = np.repeat(np.arange(M), np.diff(rp))
    ci2 = newcol[np.lexsort((newcol, rows))].astype(np.int32)
    return (M, N, rp, ci2), lambda y: np.concatenate([y[:, M:], y[:, :M]], axis=1)


def high_degree_code(hi_groups, hi_deg):
    from ldpc_ece535a import codes
    table = codes.dvbs2_like_table(3, K=5400, N=7200, hi_groups=hi_groups, hi_deg=hi_deg,
                                   lo_deg=3)
    return codes.ira_from_table(table, 5400, 7200)


HIGH_DEGREE = {"dc14": (3, 8), "dc20": (5, 12)}
BATCHES = (1, 63, 65, 300, 5000)
EDGES = {"non_finite": non_finite_frames, "zeros": zero_frames, "quantised": quantised_frames,
         "overflow": overflow_frames, "tiny": tiny_frames}
SPECIAL = ("c_32x64", "f_64x128", "s_48x96")
ET_CASES = ("c_32x64", "g_250x256", "r_40x300")
REFERENCE_H = "reference_h"


def special_frames(c):
    """tests/test_gpu_shapes.py's special samples on the case's frames."""
    y = np.array(c.frames)
    y[::7, 3] = np.inf
    y[1::5, 10] = -np.inf
    y[2::9, 20] = np.nan
    y[3::4, 30:34] = 0.0
    y[5::8, 40:44] = -0.0
    y[6::11, 50] = 45.0
    y[7::13, 51] = -45.0
    return y


def _reference_case():
    H = default_h()
    return sc.Case(REFERENCE_H, True, lambda: np.array(H))


def _build():
    S = {}

    def add(name, fn):
        assert name not in S, name
        S[name] = fn

    for n in sc.SMALL + sc.LARGE:
        add("shape/" + n, lambda n=n: Set("shape/" + n, sc.CASES[n].frames, sc.CAP,
                                          H=sc.CASES[n].H))
    for n in ET_CASES:
        add("shape/%s/et5" % n, lambda n=n: Set("shape/%s/et5" % n, sc.CASES[n].frames, sc.CAP,
                                                et=5, H=sc.CASES[n].H))
    for n in SPECIAL:
        add("special/" + n, lambda n=n: Set("special/" + n, special_frames(sc.CASES[n]), sc.CAP,
                                            H=sc.CASES[n].H))
    for db in (0, 2, 4):
        for cap in (5, 50):
            name = "default/db%d/cap%d" % (db, cap)
            add(name, lambda name=name, db=db, cap=cap: Set(
                name, golden("frames_default.npz")["db%d_llr" % db], cap, H=default_h()))
    for et in (1, 5):
        name = "persistent/%s/et%d" % (REFERENCE_H, et)
        add(name, lambda name=name, et=et: Set(name, _reference_case().frames, sc.CAP, et=et,
                                               H=default_h()))
    add("persistent/c_32x64/et5", lambda: Set("persistent/c_32x64/et5", sc.CASES["c_32x64"].frames,
                                              sc.CAP, et=5, H=sc.CASES["c_32x64"].H))
    add("dvb/knobs", lambda: Set("dvb/knobs", ira_noisy(dvb_code(), 96, 91, 1.5), 30,
                                 csr=dvb_code()))

    def info_first():
        csr2, permute = dvb_info_first()
        return Set("dvb/info_first", permute(ira_noisy(dvb_code(), 96, 17, 1.5)), 30, csr=csr2)
    add("dvb/info_first", info_first)
    for tag, (g, d) in HIGH_DEGREE.items():
        for db in (3, 6):
            name = "%s/%ddB" % (tag, db)
            add(name, lambda name=name, g=g, d=d, db=db: Set(
                name, ira_noisy(high_degree_code(g, d), 96, d, float(db)), 40,
                csr=high_degree_code(g, d)))
    for B in BATCHES:
        for et in (1, 5):
            name = "batch/%d/et%d" % (B, et)
            add(name, lambda name=name, B=B, et=et: Set(name, mixed_frames(default_h(), B, B), 50,
                                                        et=et, H=default_h()))
    for tag, fn in EDGES.items():
        add("edge/" + tag, lambda tag=tag, fn=fn: Set("edge/" + tag, fn(), 20, H=default_h()))
    add("edge/degree_one_row", lambda: Set("edge/degree_one_row", sc.CASES["e_24x64"].frames,
                                           sc.CAP, H=degree_one_row_code()))
    return S


SETS = _build()
_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = SETS[name]()
    return _CACHE[name]
