"""The fixed-point layered min-sum contract ("q8": include/ldpc_hip.h, DESIGN
section 7d), restated in numpy.

`decode` is what tests hold the kernels (csrc/ldpc_layered.hip,
ldpc_decode_layered_q8*) to, value for value; `decode_scalar` is a second
transcription in plain Python integers, one place at a time, that pins it
(tests/test_layered_q8_host.py).  num is an integer in [1, 16].

    tx_i = in_i * polarity                    (float32; negated on its own)
    v_i  = (-tx_i) * llr_scale                (one float32 multiply)
    Lc_i = 0 if v_i is NaN, else clamp(rint(v_i), -127, 127)   (ties to even)
    LQ[i] = Lc_i;  R[e] = 0
    for it = 0, 1, ...:
      for layer l, for every row j of layer l, edges e_k in ascending column c_k:
        q_k  = LQ[c_k] - R[e_k]
        s_k  = -1 if q_k < 0 else +1
        P    = s_0 * ... * s_{d-1}
        lo_k = min(127, |q_t| for t != k)
        R[e_k]  = (P * s_k) * ((lo_k * num + 8) >> 4)
        LQ[c_k] = q_k + R[e_k]
      vhat_i = LQ[i] < 0;  used = it + 1
      if used == max_iters: stop
      if used % et_period == 0 and the syndrome weight of vhat is 0: stop
    llr = (float32)LQ

`decode` is vectorised over the frames and over the rows of a layer (they
share no column, so their updates commute); the layers and the iterations are
Python loops in the order above.  All state is int32; the contract's int8 / int16
hold the same values (|R| <= 127, |LQ| <= 127 (dv + 1))."""
import numpy as np

from layered_ref import rows_in_order

KEYS = ("bits", "packed", "iters", "synd")
PAD = 32767        # a place past a row's degree: sign +, never below a minimum


def quantise(y, llr_scale, polarity=1.0):
    """(B, N) float32 samples -> Lc, int32."""
    with np.errstate(all="ignore"):
        tx = np.asarray(y, np.float32) * np.float32(polarity)
        v = (-tx) * np.float32(llr_scale)
        r = np.clip(np.rint(v), np.float32(-127), np.float32(127))
        return np.where(np.isnan(v), np.float32(0), r).astype(np.int32)


def _layers(csr, plan):
    """Per layer: (rows, C, Ei, V) -- the columns and edge indices of its rows,
    padded to the layer's largest degree, and which places are real."""
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    plan = np.asarray(plan)
    out = []
    for l in range(int(plan.max()) + 1 if plan.size else 0):
        rows = np.nonzero(plan == l)[0]
        deg = rp[rows + 1] - rp[rows]
        rows, deg = rows[deg > 0], deg[deg > 0]
        if rows.size == 0:
            continue
        k = np.arange(int(deg.max()))[None, :]
        V = k < deg[:, None]
        Ei = np.where(V, rp[rows][:, None] + k, 0)
        out.append((rows, ci[Ei], Ei, V))
    return out


def _syndrome(vhat, rp, ci):
    """Weights (B,) of the syndromes of vhat (B, N) bool."""
    cs = np.zeros((vhat.shape[0], ci.size + 1), np.int64)
    np.cumsum(vhat[:, ci], axis=1, out=cs[:, 1:])
    return ((cs[:, rp[1:]] - cs[:, rp[:-1]]) & 1).sum(axis=1)


def decode(csr, plan, y, max_iters, num=16, llr_scale=8.0, et_period=1, polarity=1.0):
    """y: (B, N) float32 samples.  Returns bits, packed, iters, synd and llr
    (the float posteriors), as the decoder's host entry point does."""
    M, N, rp, ci = csr
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    num = int(num)
    assert 1 <= num <= 16
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    layers = _layers(csr, plan)
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), llr=np.zeros((B, N), np.float32))
    LQ = quantise(y, llr_scale, polarity)
    R = np.zeros((B, int(rp[M])), np.int32)
    live = np.arange(B)                   # frames still decoding; LQ, R hold those alone
    for it in range(max_iters):
        for rows, C, Ei, V in layers:
            q = np.where(V, LQ[:, C] - R[:, Ei], PAD)          # (B, rows, places)
            neg = q < 0
            odd = (neg.sum(axis=2) & 1).astype(bool)           # P < 0
            mag = np.abs(q)
            at = mag.argmin(axis=2)
            m1 = np.take_along_axis(mag, at[..., None], axis=2)
            rest = mag.copy()
            np.put_along_axis(rest, at[..., None], PAD, axis=2)
            m2 = rest.min(axis=2, keepdims=True)
            mine = np.arange(q.shape[2])[None, None, :] == at[..., None]
            lo = np.minimum(np.where(mine, m2, m1), 127)
            m = (lo * num + 8) >> 4
            Rn = np.where(odd[..., None] ^ neg, -m, m)
            R[:, Ei[V]] = Rn[:, V]
            LQ[:, C[V]] = (q + Rn)[:, V]
        used = it + 1
        last = used == max_iters
        if not (last or used % et_period == 0):
            continue
        vhat = LQ < 0
        weight = _syndrome(vhat, rp, ci)
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


def _quantise_scalar(sample, llr_scale, polarity):
    with np.errstate(all="ignore"):
        tx = np.float32(sample) * np.float32(polarity)
        v = np.float32(-tx) * np.float32(llr_scale)
    if v != v:
        return 0
    if v >= 127:
        return 127
    if v <= -127:
        return -127
    return int(round(float(v)))           # Python rounds halves to even


def decode_scalar(csr, plan, y, max_iters, num=16, llr_scale=8.0, et_period=1, polarity=1.0):
    """The pseudo-code again in Python integers: one frame, one row, one place
    at a time."""
    M, N, rp, ci = csr
    rp = [int(v) for v in rp]
    ci = [int(v) for v in ci]
    num = int(num)
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    order = [int(j) for j in rows_in_order(plan)]
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), llr=np.zeros((B, N), np.float32))
    for b in range(B):
        LQ = [_quantise_scalar(y[b, i], llr_scale, polarity) for i in range(N)]
        R = [0] * rp[M]
        used = weight = 0
        while True:
            for j in order:
                es = range(rp[j], rp[j + 1])
                q = [LQ[ci[e]] - R[e] for e in es]
                s = [-1 if v < 0 else 1 for v in q]
                P = 1
                for v in s:
                    P *= v
                for k, e in enumerate(es):
                    lo = 127
                    for t in range(len(q)):
                        if t != k and abs(q[t]) < lo:
                            lo = abs(q[t])
                    R[e] = (P * s[k]) * ((lo * num + 8) >> 4)
                    LQ[ci[e]] = q[k] + R[e]
            vhat = [int(v < 0) for v in LQ]
            used += 1
            weight = sum(sum(vhat[ci[e]] for e in range(rp[j], rp[j + 1])) & 1 for j in range(M))
            if used == max_iters or (used % et_period == 0 and weight == 0):
                break
        out["bits"][b] = vhat
        out["iters"][b] = used
        out["synd"][b] = weight
        out["llr"][b] = np.array(LQ, np.float32)
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out


# ---- what the q8 tests share -------------------------------------------------------

def a16(x):
    return (x + 15) // 16 * 16


def frame_bytes(N, E):
    """The header's formula for one frame's LDS."""
    return a16(2 * N) + a16(E) + 128


def plant_ties(y, llr_scale):
    """Samples whose scaled value is exactly +-0.5, +-1.5 and +-127.5 (the tie
    and clamp rules; llr_scale a power of two), on strides of frames.  In place."""
    for k, v in enumerate((0.5, -0.5, 1.5, -1.5, 127.5, -127.5)):
        y[k::6, 5 + k] = np.float32(-v / llr_scale)
    return y


# The three codes the float decoder refuses at PREC_F32 (Z = 1024, mb = 4).
def large_base(nb):
    """qc_dual_diagonal(4, nb, 1024, 3, seed): nb = 12 is larger than a float
    frame (N = 12288, E = 31744), nb = 24 has E = 68608 > 65535."""
    from ldpc_ece535a import codes
    return codes.qc_dual_diagonal(4, nb, 1024, 3, 20 + nb)


def boundary_base(entries):
    """Z = 1024, mb = 4, nb = 48 (N = 49152): the parity part (7 entries), then
    the information columns filled column by column, in the manner of
    qc_cases.boundary_base.  63 entries make a frame of 98304 + 64512 + 128 =
    162944 bytes, 64 make 163968."""
    S = np.full((4, 48), -1, np.int32)
    for r in range(4):
        S[r, r] = 0
        if r >= 1:
            S[r, r - 1] = 0
    n = 7
    for c in range(4, 48):
        for r in ((c % 4), ((c + 1) % 4)):
            if n < entries:
                S[r, c] = (37 * n + 11) % 1024
                n += 1
    assert int((S >= 0).sum()) == entries
    return S
