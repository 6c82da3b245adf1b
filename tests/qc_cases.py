"""The quasi-cyclic codes and frames the QC tests share (tests/test_qc_host.py,
tests/test_gpu_qc.py).  All base matrices are synthetic: qc_dual_diagonal's
seeded draws and a hand-built one for the degree limits."""
import numpy as np

# name -> (mb, nb, Z, info_deg, seed), N / E, (fseed, B, dB, cap, precision)
TABLE = {
    "A": ((6, 12, 64, 3, 1), (768, 1856), (101, 48, 2.0, 20, 0)),
    "B": ((12, 24, 27, 3, 2), (648, 1593), (102, 48, 2.0, 20, 0)),       # Z below a wave
    "C": ((6, 30, 96, 3, 3), (2880, 7968), (103, 32, 5.0, 15, 0)),       # long rows, 1.5 waves
    "D": ((4, 10, 384, 3, 4), (3840, 9600), (104, 16, 3.0, 12, 0)),      # six waves
    "E": ((20, 40, 1, 3, 5), (40, 99), (105, 64, 1.0, 20, 0)),           # Z = 1
    "F": ((2, 6, 1024, 2, 6), (6144, 11264), (106, 8, 3.0, 10, 1)),      # 1024 threads
}
G_FRAMES = (107, 256, 5.0, 20)   # fseed, B, dB, cap


def base_of(name):
    """(base, Z) of a case."""
    from ldpc_ece535a import codes
    if name == "G":
        return degree_limit_base(), 5
    mb, nb, Z, info_deg, seed = TABLE[name][0]
    return codes.qc_dual_diagonal(mb, nb, Z, info_deg, seed), Z


def degree_limit_base():
    """Z = 5, mb = 4, nb = 35: the parity diagonal at shift 0 with the
    sub-diagonal in block rows 1 and 2 only (block row 3 and block column 3
    have degree 1); block row 0 holds all 31 information block columns (degree
    32, shifts 0 and Z - 1 among them); every information block column has one
    more circulant, in block row 1 (10 of them: degree 12) or 2 (21: degree 23)."""
    S = np.full((4, 35), -1, np.int32)
    for r in range(4):
        S[r, r] = 0
    S[1, 0] = S[2, 1] = 0
    for c in range(4, 35):
        S[0, c] = (3 * c) % 5
        S[1 if c % 3 == 0 else 2, c] = (2 * c + 1) % 5
    return S


def rolled(base, Z):
    """The expansion from rolled identity blocks: dense H and its CSR."""
    base = np.asarray(base)
    mb, nb = base.shape
    H = np.zeros((mb * Z, nb * Z), np.uint8)
    eye = np.eye(Z, dtype=np.uint8)
    for r in range(mb):
        for c in range(nb):
            if base[r, c] >= 0:   # row i has its one at column (i + s) mod Z
                H[r * Z:(r + 1) * Z, c * Z:(c + 1) * Z] = np.roll(eye, int(base[r, c]), axis=1)
    rows, cols = np.nonzero(H)
    rp = np.zeros(mb * Z + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return H, (mb * Z, nb * Z, np.cumsum(rp).astype(np.int32), cols.astype(np.int32))


def frames(csr, fseed, B, db):
    """B noisy BPSK codewords of random information bits."""
    from ldpc_ece535a import codes
    M, N = csr[0], csr[1]
    rng = np.random.Generator(np.random.PCG64(fseed))
    info = rng.integers(0, 2, (B, N - M), np.uint8)
    cw = codes.qc_encode(csr, info)
    y = 2.0 * cw - 1.0 + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(cw.shape)
    return y.astype(np.float32)


def plant_special(y):
    """The special samples of tests/test_gpu_layered.py's _frames720, on
    strides of frames: +-inf, NaN, runs of +0.0 and of -0.0.  In place."""
    y[::7, 3] = np.inf
    y[1::5, 10] = -np.inf
    y[2::9, 20] = np.nan
    y[3::4, 30:34] = 0.0
    y[5::8, 400:404] = -0.0
    return y


def block_rows(mb, Z):
    return np.repeat(np.arange(mb, dtype=np.int32), Z)


# the LDS boundary: Z = 384, mb = 4, nb = 12; 39 base entries make a double
# frame of 8 * (4608 + 14976) + 4608 + 128 = 161408 bytes, 40 make 164480
def boundary_base(entries):
    S = np.full((4, 12), -1, np.int32)
    for r in range(4):
        S[r, r] = 0
        if r >= 1:
            S[r, r - 1] = 0
    n = 7
    cells = [(r, c) for c in range(4, 12) for r in range(4)] + [(2, 0), (3, 0), (3, 1)]
    for r, c in cells:   # the information part, then below the sub-diagonal
        if n < entries:
            S[r, c] = (37 * n + 11) % 384
            n += 1
    assert int((S >= 0).sum()) == entries
    return S
