"""Plain min-sum (the reference's decodeLogDomainSimple), restated in numpy
and generic over the arithmetic type.

    tx_i  = in_i * polarity                    (float; negated as an operation of its own)
    Lci_i = (Real)(-tx_i);  Lq[e] = Lci[col(e)];  Lr[e] = 0
    for it = 0, 1, ...:
      for every row r, edges e_k in ascending column:
        s_k  = (Lq[e_k] > 0) - (Lq[e_k] < 0)
        P    = s_0 * ... * s_{d-1}
        lo_k = BIG;  for t != k, ascending:  if (|Lq[e_t]| < lo_k) lo_k = |Lq[e_t]|
        Lr[e_k] = (Real)(P * s_k) * lo_k
      for every column c, edges e_k in ascending row:
        s = 0;  for k ascending:  s = s + Lr[e_k]
        LQ[c] = Lci[c] + s
        Lq[e_k] = LQ[c] - Lr[e_k]
        vhat[c] = LQ[c] < 0
      used = it + 1
      if used == max_iters: stop
      if used % et_period == 0 and the syndrome weight of vhat is 0: stop

BIG is the largest finite Real (DBL_MAX / FLT_MAX).  At Real = float64 this is
oracle/ldpc_oracle.c's min-sum, which tests/test_minsum_f32_host.py holds it
to bit for bit; at Real = float32 it is the contract of the decoder's f32
min-sum (precision 1, method 0) and equals the oracle's float restatement.

`decode` is vectorised over frames and over the rows (columns) of one degree;
the places of a row and the checks of a column are Python loops in the order
above, and each numpy call is one IEEE operation per element (numpy never
contracts a multiply and an add).  `accumulate` and `descending` are
mutations for the tests that show the inputs can tell such variants apart:
the column sum taken in double and rounded once, or taken from the last row
to the first."""
import numpy as np

KEYS = ("bits", "packed", "iters", "synd")


def _groups(ptr):
    """[(members, (n, d) index matrix)] for the members of each length d."""
    ptr = np.asarray(ptr, np.int64)
    deg = np.diff(ptr)
    out = []
    for d in np.unique(deg):
        who = np.nonzero(deg == d)[0]
        out.append((who, ptr[who][:, None] + np.arange(int(d))[None, :]))
    return out


def decode(csr, y, max_iters, Real=np.float32, et_period=1, polarity=1.0, accumulate=None,
           descending=False):
    """y: (B, N) float32 samples.  Returns bits, packed, iters, synd and post
    (the posteriors cast to float32), as oracle.decode_batch does, and
    post_real (the posteriors as Real)."""
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    E = int(rp[M])
    BIG = np.finfo(Real).max
    Acc = Real if accumulate is None else accumulate
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    rows = _groups(rp)
    # the edges column by column, ascending row within a column
    erow = np.repeat(np.arange(M), np.diff(rp))
    by_col = np.lexsort((erow, ci))
    cp = np.zeros(N + 1, np.int64)
    np.add.at(cp, ci + 1, 1)
    cols = [(c, by_col[k]) for c, k in _groups(np.cumsum(cp))]
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), post=np.zeros((B, N), np.float32),
               post_real=np.zeros((B, N), Real))
    with np.errstate(all="ignore"):
        tx = y * np.float32(polarity)
        Lci = (-tx).astype(Real)
        Lq = Lci[:, ci]
        Lr = np.zeros((B, E), Real)
        LQ = np.zeros((B, N), Real)
        live = np.arange(B)               # frames still decoding; the arrays hold those alone
        for it in range(max_iters):
            for _, e in rows:
                d = e.shape[1]
                if d == 0:
                    continue
                q = Lq[:, e]
                s = (q > 0).astype(np.int32) - (q < 0).astype(np.int32)
                P = np.prod(s, axis=2, dtype=np.int32)
                mag = np.abs(q)
                lo = np.full(q.shape, BIG, Real)
                for t in range(d):        # every place k != t takes |q_t| if it is smaller
                    v = mag[:, :, t:t + 1]
                    m = v < lo
                    m[:, :, t] = False
                    lo = np.where(m, v, lo)
                Lr[:, e] = (P[:, :, None] * s).astype(Real) * lo
            for c, e in cols:
                d = e.shape[1]
                s = np.zeros((live.size, c.size), Acc)
                for k in (range(d - 1, -1, -1) if descending else range(d)):
                    s = s + Lr[:, e[:, k]]
                lq = Lci[:, c] + s.astype(Real)
                LQ[:, c] = lq
                if d:
                    Lq[:, e] = lq[:, :, None] - Lr[:, e]
            used = it + 1
            last = used == max_iters
            if not (last or used % et_period == 0):
                continue
            vhat = LQ < 0
            weight = np.zeros(live.size, np.int64)
            for _, e in rows:
                weight += (vhat[:, ci[e]].sum(axis=2) & 1).sum(axis=1)
            stop = np.ones(live.size, bool) if last else weight == 0
            idx = live[stop]
            out["bits"][idx] = vhat[stop]
            out["iters"][idx] = used
            out["synd"][idx] = weight[stop]
            out["post"][idx] = LQ[stop].astype(np.float32)
            out["post_real"][idx] = LQ[stop]
            keep = ~stop
            live, Lci, Lq, Lr, LQ = live[keep], Lci[keep], Lq[keep], Lr[keep], LQ[keep]
            if live.size == 0:
                break
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out
