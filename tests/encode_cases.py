"""The codes and data of tests/test_gpu_encode_shapes.py: what the device
encoders (csrc/ldpc_aux.hip: k_encode_small<KW>, k_encode_ira) are run on.

Small codes (K <= 256, any M): sparse H with every column of weight 3 and the
rows as even as a greedy fill makes them, drawn from a seed whose matrix has
rank M (tests/test_encode_cases_host.py checks it on the CPU).  The context
reorders the columns; the reference (tests/gf2_ref.py) encodes with the
context's own H.

IRA codes: the accumulator staircase in columns 0..M-1 and a seeded
information part, as CSR."""
import numpy as np

# (M, N, seed): what the shape covers
SMALL = [
    (64, 128, 0),     # K = 64: one full data word
    (63, 128, 0),     # K = 65: KW = 2, one bit in the second word
    (64, 192, 0),     # K = 128: two full words
    (64, 193, 0),     # K = 129: KW = 3
    (64, 256, 0),     # K = 192: three full words
    (31, 256, 0),     # K = 225: KW = 4, partial last word
    (65, 130, 0),     # M = 65: a second pass of the row loop
    (200, 256, 0),    # K = 56: four passes of the row loop
    (40, 296, 0),     # K = 256: KW = 4 full, the K <= 256 boundary; N beyond the small decoders
    (300, 500, 0),    # K = 200: M > 256, five passes
]
GOLDEN = "hData2"     # (50, 100), K = 50: the fixture no encoder test used
REFUSED = (41, 298, 0)   # K = 257: past the small rule, and no staircase

BATCHES = [1, 3, 333]


def small_code(M, N, seed):
    """(M, N) uint8 H: column by column, three distinct rows among the lightest
    so far, ties broken by the seed."""
    rng = np.random.Generator(np.random.PCG64([M, N, seed]))
    H = np.zeros((M, N), np.uint8)
    weight = np.zeros(M, np.int64)
    for c in range(N):
        rows = np.lexsort((rng.random(M), weight))[:3]
        H[rows, c] = 1
        weight[rows] += 1
    return H


def data_for(K, B, seed=0):
    """(B, K) data bits.  B = 1: a random frame; B = 3: all-zero, all-one,
    random; larger: those, then the K unit vectors (which read the encoder's
    matrix back column by column), then random frames."""
    rng = np.random.Generator(np.random.PCG64([K, B, seed]))
    d = rng.integers(0, 2, (B, K), dtype=np.uint8)
    if B >= 3:
        d[0] = 0
        d[1] = 1
    if B >= K + 3:
        d[2:K + 2] = np.eye(K, dtype=np.uint8)
    return d


# ---- IRA --------------------------------------------------------------------------

# (M, K, kind).  M < 256: threads without a row, one row a thread; M = 256: every
# thread one row; 257, 511, 1000: two to four rows a thread, ragged last segments
IRA = [
    (100, 300, "random"),
    (256, 300, "random"),
    (257, 300, "random"),
    (511, 700, "empty_rows"),    # every third row has no information bit
    (1000, 257, "one_row"),      # all information ones in row 613: 30 columns, the row-degree
                                 # limit of a context (32) less the staircase; the rest empty
]
IRA_BATCHES = [1, 37]


def ira_code(M, K, kind, seed=0):
    """CSR (M, N, row_ptr, col_idx): row j holds parity columns j - 1 and j and
    its information columns (>= M), ascending."""
    rng = np.random.Generator(np.random.PCG64([M, K, seed]))
    N = M + K
    info = [[] for _ in range(M)]
    if kind == "one_row":
        info[613 % M] = sorted(int(c) for c in rng.choice(K, 30, replace=False))
    else:
        allowed = np.arange(M)
        if kind == "empty_rows":
            allowed = allowed[allowed % 3 != 1]
        for c in range(K):
            for j in rng.choice(allowed, 3, replace=False):
                info[int(j)].append(c)
    rp, ci = [0], []
    for j in range(M):
        row = ([j - 1] if j else []) + [j] + [M + c for c in sorted(info[j])]
        ci += row
        rp.append(len(ci))
    return M, N, np.array(rp, np.int32), np.array(ci, np.int32)
