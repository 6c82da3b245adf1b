"""Sum-product (the reference's decodeSumProductSoft, oracle/ldpc_oracle.c
orc_sumproduct_sparse), restated in numpy, generic over the arithmetic type
and over the two functions a host cannot take from the device:

    tx_i = in_i * polarity                      (float)
    r_i  = (Real)(-tx_i);  Q[e] = r[col(e)]
    for it = 0, 1, ...:
      t[e]  = tanh_half(Q[e])                                   <- callable
      for every row, edges e_k in ascending column:
        T_k = 1;  for j != k, ascending:  T_k = T_k * t[e_j]
      Ec[e] = check_msg(T[e])                                   <- callable
      for every column c, edges e_k in ascending row:
        L = 0;    for k ascending:          L = L + (Ec[e_k] + r_c)
        Q[e_k] = 0;  for j != k, ascending:  Q[e_k] = Q[e_k] + (Ec[e_j] + r_c)
      vhat_c = L <= 0
      used = it + 1
      if used % et_period == 0 and the syndrome weight of vhat is 0: stop
      if used == max_iters: stop

tanh_half(m) stands for tanh(m / 2) and check_msg(T) for
log((1 + T) / (1 - T)); both take and return arrays of Real.  Everything else
is one IEEE operation per element (numpy never contracts a multiply and an
add), which is what the kernels compute with contraction off.  With glibc's
functions (oracle.tanh_half, oracle.log_ratio) at float64 this is the C
oracle bit for bit (tests/test_sumproduct_ref_host.py); with the device's
functions (ldpc_math_probe) it is the contract of the decoder's inexact
precisions on every route whose kernels make scalar Math<PREC> calls
(tests/test_gpu_sumproduct_inexact.py).

`reverse_product` and `sum_from_r` are mutations for the tests that show the
inputs can tell such variants apart: the row product taken from the last
column to the first, and the column sums started from r instead of 0."""
import numpy as np

from minsum_ref import _groups

KEYS = ("bits", "packed", "iters", "synd")


def decode(csr, y, max_iters, tanh_half, check_msg, Real=np.float64, et_period=1, polarity=1.0,
           reverse_product=False, sum_from_r=False):
    """y: (B, N) float32 samples.  Returns bits, packed, iters, synd, post (the
    posteriors cast to float32, as oracle.decode_batch and the decoder return
    them) and post_real (the posteriors as Real)."""
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    E = int(rp[M])
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    rows = _groups(rp)
    erow = np.repeat(np.arange(M), np.diff(rp))
    by_col = np.lexsort((erow, ci))
    cp = np.zeros(N + 1, np.int64)
    np.add.at(cp, ci + 1, 1)
    cols = [(c, by_col[k]) for c, k in _groups(np.cumsum(cp))]
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), post=np.zeros((B, N), np.float32),
               post_real=np.zeros((B, N), Real))

    def call(f, x):
        z = np.asarray(f(np.ascontiguousarray(x, Real)))
        assert z.dtype == Real and z.shape == x.shape, (z.dtype, z.shape)
        return z

    with np.errstate(all="ignore"):
        tx = y * np.float32(polarity)
        r = (-tx).astype(Real)
        Q = r[:, ci]
        live = np.arange(B)               # frames still decoding; the arrays hold those alone
        for it in range(max_iters):
            t = call(tanh_half, Q)
            T = np.ones((live.size, E), Real)
            for _, e in rows:
                d = e.shape[1]
                order = range(d - 1, -1, -1) if reverse_product else range(d)
                for k in range(d):
                    p = np.ones((live.size, e.shape[0]), Real)
                    for j in order:
                        if j != k:
                            p = p * t[:, e[:, j]]
                    T[:, e[:, k]] = p
            Ec = call(check_msg, T)
            L = np.zeros((live.size, N), Real)
            for c, e in cols:
                d = e.shape[1]
                rc = r[:, c]
                term = [Ec[:, e[:, k]] + rc for k in range(d)]
                s = rc.copy() if sum_from_r else np.zeros_like(rc)
                for k in range(d):
                    s = s + term[k]
                L[:, c] = s
                for k in range(d):
                    m = rc.copy() if sum_from_r else np.zeros_like(rc)
                    for j in range(d):
                        if j != k:
                            m = m + term[j]
                    Q[:, e[:, k]] = m
            used = it + 1
            vhat = L <= 0
            weight = np.zeros(live.size, np.int64)
            for _, e in rows:
                weight += (vhat[:, ci[e]].sum(axis=2) & 1).sum(axis=1)
            stop = (weight == 0) if used % et_period == 0 else np.zeros(live.size, bool)
            if used == max_iters:
                stop = np.ones(live.size, bool)
            idx = live[stop]
            out["bits"][idx] = vhat[stop]
            out["iters"][idx] = used
            out["synd"][idx] = weight[stop]
            out["post"][idx] = L[stop].astype(np.float32)
            out["post_real"][idx] = L[stop]
            keep = ~stop
            live, r, Q = live[keep], r[keep], Q[keep]
            if live.size == 0:
                break
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out


# ---- an enclosure for routes that have no elementwise restatement -----------------------------------

_LD = np.longdouble
# what long double arithmetic itself may add to a bound (2^-64 per operation,
# a handful of operations per step)
_SLACK = _LD(2.0) ** -60


def _step(x, k):
    """the double k units in the last place above (k < 0: below) x, in the
    order of the reals; NaN stays NaN"""
    x = np.ascontiguousarray(x, np.float64)
    i = x.view(np.int64)
    key = np.where(i < 0, np.int64(-2 ** 63) - i, i) + np.int64(k)
    back = np.where(key < 0, np.int64(-2 ** 63) - key, key)
    return np.where(np.isnan(x), x, back.view(np.float64))


def _out(lo, hi, rel):
    """the interval widened outwards by the relative amount rel (+ slack)"""
    w = _LD(rel) + _SLACK
    return lo - np.abs(lo) * w, hi + np.abs(hi) * w


def enclosure_cap1(csr, y, tanh_half_glibc):
    """The lowest and highest posterior (as float32) a one-iteration
    sum-product decode of the finite frames y can return in double arithmetic
    when
      * every tanh(m / 2) lies within 3 ulp of glibc's value (tanh_half_glibc)
        and within [-1, 1],
      * every step of the row product is rounded once,
      * every check message lies within 3 ulp of the log of a ratio that lies
        within 1 ulp of (1 + T) / (1 - T),
      * every addition of the column sum is rounded once.
    tanh and log((1 + T) / (1 - T)) are monotone, so the extremes are reached
    at the ends of each interval; they are evaluated in long double, each step
    widened by the rounding it stands for (2^-53 relative for one rounding of a
    double, 2^-52 for one ulp, 3 spacings of the double for 3 ulp) and by
    2^-60 for long double's own error.  A bound that comes out NaN (inf - inf)
    is no bound.  Returns (lo, hi), each (B, N) float32."""
    assert np.finfo(_LD).nmant >= 63
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    assert np.isfinite(y).all()
    B = y.shape[0]
    E = int(rp[M])
    erow = np.repeat(np.arange(M), np.diff(rp))
    with np.errstate(all="ignore"):
        r = (-y).astype(np.float64)
        t = np.asarray(tanh_half_glibc(np.ascontiguousarray(r[:, ci])), np.float64)
        tl = np.clip(_step(t, -3), -1.0, 1.0).astype(_LD)
        th = np.clip(_step(t, 3), -1.0, 1.0).astype(_LD)
        Tl = np.ones((B, E), _LD)
        Th = np.ones((B, E), _LD)
        for _, e in _groups(rp):
            d = e.shape[1]
            for k in range(d):
                pl = np.ones((B, e.shape[0]), _LD)
                ph = pl.copy()
                for j in range(d):
                    if j == k:
                        continue
                    a, b = tl[:, e[:, j]], th[:, e[:, j]]
                    c = np.stack([pl * a, pl * b, ph * a, ph * b])
                    pl, ph = _out(c.min(axis=0), c.max(axis=0), 2.0 ** -53)
                Tl[:, e[:, k]] = np.maximum(pl, -1)
                Th[:, e[:, k]] = np.minimum(ph, 1)
        ql, _ = _out((1 + Tl) / (1 - Tl), (1 + Tl) / (1 - Tl), 2.0 ** -52)
        _, qh = _out((1 + Th) / (1 - Th), (1 + Th) / (1 - Th), 2.0 ** -52)
        El, Eh = np.log(np.maximum(ql, 0)), np.log(qh)
        El = El - 3 * np.spacing(np.abs(El.astype(np.float64))).astype(_LD) - np.abs(El) * _SLACK
        Eh = Eh + 3 * np.spacing(np.abs(Eh.astype(np.float64))).astype(_LD) + np.abs(Eh) * _SLACK
        by_col = np.lexsort((erow, ci))
        cp = np.zeros(N + 1, np.int64)
        np.add.at(cp, ci + 1, 1)
        lo = np.zeros((B, N), _LD)
        hi = np.zeros((B, N), _LD)
        for c, k in _groups(np.cumsum(cp)):
            e = by_col[k]
            rc = r[:, c].astype(_LD)
            sl = np.zeros((B, c.size), _LD)
            sh = sl.copy()
            for j in range(e.shape[1]):
                a, b = _out(El[:, e[:, j]] + rc, Eh[:, e[:, j]] + rc, 2.0 ** -53)
                sl, sh = _out(sl + a, sh + b, 2.0 ** -53)
            lo[:, c], hi[:, c] = sl, sh
        lo = np.where(np.isnan(lo), -np.inf, lo).astype(np.float32)
        hi = np.where(np.isnan(hi), np.inf, hi).astype(np.float32)
    return lo, hi


def assert_enclosed(out, lo, hi, what):
    """posteriors inside [lo, hi]; decisions equal wherever 0 is outside it"""
    post = np.asarray(out["llr"], np.float32)
    inside = (post >= lo) & (post <= hi)
    assert inside.all(), "%s: %d posteriors outside the enclosure, first at %s: %r not in [%r, %r]" % (
        what, (~inside).sum(), np.argwhere(~inside)[0], post[~inside][0], lo[~inside][0],
        hi[~inside][0])
    one, zero = hi < 0, lo > 0
    assert (out["bits"][one] == 1).all() and (out["bits"][zero] == 0).all(), what
    return float((one | zero).mean())
