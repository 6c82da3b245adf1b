"""The rate-matching contract (include/ldpc_hip.h), restated
in numpy: what tests hold ldpc_plan_rate_match, ldpc_rate_match,
ldpc_rate_recover and the fused layered decodes to.

Transmit position p in [0, N) is column M + p for p < K = N - M and column
p - K otherwise.  A pattern (punct, filler, ncb): positions [0, punct) are never
sent, positions [K - filler, K) are known zeros and never sent, and the
circular buffer is positions [punct, punct + ncb), ncb = 0 meaning N - punct.

`walk` is the literal statement -- one buffer offset at a time from k0, mod
ncb, skipping the fillers, until E positions are emitted; `closed` is the
closed form the library computes with; `recover` takes a column's terms in
sample order (transmissions ascending, e ascending within one), the first as it
is and every later one a float32 add."""
import numpy as np


def resolve(M, N, punct, filler, ncb):
    """(K, ncb, S, fs, fe) of a pattern."""
    K = N - M
    ncb = ncb if ncb else N - punct
    return K, ncb, ncb - filler, K - filler - punct, K - punct


def col_of_pos(M, N, p):
    K = N - M
    p = np.asarray(p)
    return np.where(p < K, M + p, p - K)


def walk(M, N, punct, filler, ncb, k0, E):
    """The columns of the E samples of transmission (k0, E), one step at a time."""
    K, ncb, _, _, _ = resolve(M, N, punct, filler, ncb)
    out = []
    j = k0
    while len(out) < E:
        pos = punct + j
        if not K - filler <= pos < K:
            out.append(M + pos if pos < K else pos - K)
        j = (j + 1) % ncb
    return np.array(out, np.int64)


def closed(M, N, punct, filler, ncb, k0, E):
    """The same columns by the closed form."""
    _, ncb, S, fs, fe = resolve(M, N, punct, filler, ncb)
    u0 = (k0 if k0 < fs else max(k0, fe) - filler) % S
    u = (u0 + np.arange(E, dtype=np.int64)) % S
    j = np.where(u < fs, u, u + filler)
    return col_of_pos(M, N, punct + j)


def columns(M, N, pattern, tx):
    """The column of every sample of a call, transmissions concatenated."""
    return np.concatenate([closed(M, N, *pattern, k0, E) for k0, E in tx])


def filler_columns(M, N, pattern):
    K = N - M
    return col_of_pos(M, N, np.arange(K - pattern[1], K))


def counts(M, N, pattern, tx):
    """Samples per column, -1 for a filler."""
    c = np.bincount(columns(M, N, pattern, tx), minlength=N).astype(np.int32)
    c[filler_columns(M, N, pattern)] = -1
    return c


def recover(M, N, pattern, tx, rx, polarity=1.0, unreceived_lci=2.0 ** -100):
    """rx (B, sum E) float32 -> Lci (B, N) float32.  The samples a decode takes
    are y = -Lci, at polarity 1."""
    rx = np.asarray(rx, np.float32)
    cols = columns(M, N, pattern, tx)
    assert rx.ndim == 2 and rx.shape[1] == cols.size
    with np.errstate(all="ignore"):
        tx_ = rx * np.float32(polarity)
        lci = -tx_
        out = np.full((rx.shape[0], N), np.float32(unreceived_lci), np.float32)
        out[:, filler_columns(M, N, pattern)] = np.float32(np.inf)
        have = np.zeros(N, bool)
        for i, c in enumerate(cols):
            out[:, c] = out[:, c] + lci[:, i] if have[c] else lci[:, i]
            have[c] = True
    return out


def bits_equal(a, b):
    """Bit for bit, NaN payloads and the sign of zero included."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
