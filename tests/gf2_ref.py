"""Systematic encoding by linear algebra over GF(2), in numpy.

For a parity-check matrix H = [H_p | H_d] (H_p: the first M columns) and data
d, the codeword [p | d] satisfies H_p p = H_d d.  When H_p is invertible -- the
decoder's reordered H makes it so -- p is unique, so any correct encoder gives
these bytes, whatever its method."""
import numpy as np


def eliminate(A, ncols):
    """Gauss-Jordan over GF(2) on a copy of A (uint8 0/1), pivoting in the first
    `ncols` columns from the left.  Returns (reduced A, pivot columns)."""
    A = (np.array(A, np.uint8) & 1)
    rows = A.shape[0]
    pivots = []
    r = 0
    for c in range(ncols):
        if r == rows:
            break
        hit = np.nonzero(A[r:, c])[0]
        if hit.size == 0:
            continue
        p = r + int(hit[0])
        if p != r:
            A[[r, p]] = A[[p, r]]
        others = np.nonzero(A[:, c])[0]
        others = others[others != r]
        A[others] ^= A[r]
        pivots.append(c)
        r += 1
    return A, pivots


def rank(H):
    H = np.asarray(H, np.uint8)
    return len(eliminate(H, H.shape[1])[1])


def encode(H, data):
    """(B, K) data bits -> (B, N) codewords [parity | data] of the (M, N) matrix
    H, whose first M columns must be independent."""
    H = np.asarray(H, np.uint8) & 1
    M, N = H.shape
    d = np.atleast_2d(np.asarray(data, np.uint8)) & 1
    assert d.shape[1] == N - M
    rhs = (H[:, M:].astype(np.int64) @ d.T.astype(np.int64) & 1).astype(np.uint8)   # (M, B)
    A, pivots = eliminate(np.concatenate([H[:, :M], rhs], axis=1), M)
    if pivots != list(range(M)):
        raise ValueError("the first M columns of H are dependent")
    return np.concatenate([A[:, M:].T, d], axis=1)


def syndrome(H, cw):
    """(B, M): H cw over GF(2)."""
    H = np.asarray(H, np.int64) & 1
    return (np.atleast_2d(np.asarray(cw, np.int64) & 1) @ H.T) & 1
