"""The layered normalized min-sum contract, restated in numpy.

`decode` is what tests hold the layered kernel (csrc/ldpc_layered.hip,
ldpc_decode_layered*) to, bit for bit; `decode_scalar` is a second, scalar
transcription of the same pseudo-code that pins it
(tests/test_layered_host.py).  Conventions are the reference min-sum's: Lci =
-tx, sign(0) = 0, the DBL_MAX / FLT_MAX seed, decision LQ < 0, the cap first,
then the syndrome on multiples of et_period.

    tx_i  = in_i * polarity            (float; negated as an operation of its own)
    LQ[i] = (Real)(-tx_i);  R[e] = 0
    for it = 0, 1, ...:
      for layer l, for every row j of layer l, edges e_k in ascending column c_k:
        q_k  = LQ[c_k] - R[e_k]
        s_k  = (q_k > 0) - (q_k < 0)
        P    = s_0 * ... * s_{d-1}
        lo_k = BIG;  for t != k, ascending:  if (|q_t| < lo_k) lo_k = |q_t|
        R[e_k]  = a * ((Real)(P * s_k) * lo_k)
        LQ[c_k] = q_k + R[e_k]
      vhat_i = LQ[i] < 0;  used = it + 1
      if used == max_iters: stop
      if used % et_period == 0 and the syndrome weight of vhat is 0: stop

`decode` is vectorised over frames only: rows, layers and the places of a row
are Python loops in the order above, and each numpy call is one IEEE operation
per element (numpy never contracts a multiply and an add)."""
import numpy as np

KEYS = ("bits", "packed", "iters", "synd")


def real_of(precision):
    return np.float32 if precision == 1 else np.float64


def first_fit(csr):
    """Row j goes to the lowest layer with which it shares no column."""
    M, N, rp, ci = csr
    used = [set() for _ in range(N)]
    plan = np.zeros(M, np.int32)
    for j in range(M):
        cols = ci[rp[j]:rp[j + 1]]
        taken = set().union(*[used[c] for c in cols]) if len(cols) else set()
        layer = 0
        while layer in taken:
            layer += 1
        plan[j] = layer
        for c in cols:
            used[c].add(layer)
    return plan


def rows_in_order(plan):
    """The rows layer by layer, ascending within a layer."""
    return np.argsort(np.asarray(plan), kind="stable")


def _dense(csr):
    M, N, rp, ci = csr
    H = np.zeros((M, N), np.float32)
    H[np.repeat(np.arange(M), np.diff(rp)), ci] = 1
    return H


def decode(csr, plan, y, max_iters, scale=1.0, precision=0, et_period=1, polarity=1.0):
    """y: (B, N) float32 samples.  Returns bits, packed, iters, synd and llr
    (the float posteriors), as the decoder's host entry point does."""
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    Real = real_of(precision)
    BIG = np.finfo(Real).max
    a = Real(scale)
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    order = rows_in_order(plan)
    HT = _dense(csr).T.copy()
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), llr=np.zeros((B, N), np.float32))
    with np.errstate(all="ignore"):
        tx = y * np.float32(polarity)
        LQ = (-tx).astype(Real)
        R = np.zeros((B, int(rp[M])), Real)
        live = np.arange(B)               # frames still decoding; LQ, R hold those alone
        for it in range(max_iters):
            for j in order:
                e0, e1 = rp[j], rp[j + 1]
                d = int(e1 - e0)
                if d == 0:
                    continue
                cols = ci[e0:e1]
                q = LQ[:, cols] - R[:, e0:e1]
                s = (q > 0).astype(np.int32) - (q < 0).astype(np.int32)
                P = np.prod(s, axis=1, dtype=np.int32)
                mag = np.abs(q)
                lo = np.full(q.shape, BIG, Real)
                for t in range(d):        # every place k != t takes |q_t| if it is smaller
                    v = mag[:, t:t + 1]
                    m = v < lo
                    m[:, t] = False
                    lo = np.where(m, v, lo)
                Rn = a * ((P[:, None] * s).astype(Real) * lo)
                R[:, e0:e1] = Rn
                LQ[:, cols] = q + Rn
            used = it + 1
            last = used == max_iters
            if not (last or used % et_period == 0):
                continue
            vhat = LQ < 0
            weight = (np.rint(vhat.astype(np.float32) @ HT).astype(np.int64) & 1).sum(axis=1)
            stop = np.ones(live.size, bool) if last else weight == 0
            idx = live[stop]
            out["bits"][idx] = vhat[stop]
            out["iters"][idx] = used
            out["synd"][idx] = weight[stop]
            out["llr"][idx] = LQ[stop].astype(np.float32)
            live, LQ, R = live[~stop], LQ[~stop], R[~stop]
            if live.size == 0:
                break
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out


def decode_scalar(csr, plan, y, max_iters, scale=1.0, precision=0, et_period=1, polarity=1.0):
    """The pseudo-code again, one frame, one row, one place at a time."""
    M, N, rp, ci = csr
    Real = real_of(precision)
    BIG = Real(np.finfo(Real).max)
    a = Real(scale)
    zero = Real(0)
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    order = [int(j) for j in rows_in_order(plan)]
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), llr=np.zeros((B, N), np.float32))
    with np.errstate(all="ignore"):
        for b in range(B):
            LQ = [Real(-(np.float32(y[b, i]) * np.float32(polarity))) for i in range(N)]
            R = [zero] * int(rp[M])
            used = weight = 0
            while True:
                for j in order:
                    es = range(int(rp[j]), int(rp[j + 1]))
                    q = [LQ[ci[e]] - R[e] for e in es]
                    s = [int(v > zero) - int(v < zero) for v in q]
                    P = 1
                    for v in s:
                        P *= v
                    for k, e in enumerate(es):
                        lo = BIG
                        for t in range(len(q)):
                            if t != k and abs(q[t]) < lo:
                                lo = abs(q[t])
                        R[e] = a * (Real(P * s[k]) * lo)
                        LQ[ci[e]] = q[k] + R[e]
                vhat = [int(v < zero) for v in LQ]
                used += 1
                weight = sum(sum(vhat[ci[e]] for e in range(int(rp[j]), int(rp[j + 1]))) & 1
                             for j in range(M))
                if used == max_iters or (used % et_period == 0 and weight == 0):
                    break
            out["bits"][b] = vhat
            out["iters"][b] = used
            out["synd"][b] = weight
            out["llr"][b] = np.array(LQ, Real).astype(np.float32)
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out


# ---- the codes and frames the layered tests share ---------------------------------

def ira_code(K, N, hi_groups):
    """The IRA codes of tests/test_gpu_onchip.py: (360, 720, 1), (1080, 2160, 2)."""
    from ldpc_ece535a import codes
    t = codes.dvbs2_like_table(3, K=K, N=N, hi_groups=hi_groups, hi_deg=6, lo_deg=3)
    return codes.ira_from_table(t, K, N)


def noisy(csr, B, db, seed):
    from ldpc_ece535a import codes
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, csr[1] - csr[0]), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)
