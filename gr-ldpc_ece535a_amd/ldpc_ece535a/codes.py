"""Parity-check matrices beyond the reference's hard-coded 32x64 H.

The reference decodes one fixed 32x64 code held as dense uBLAS matrices
(lib/ldpc_decoder_cb_impl.cc:60-106).  SURVEY 8(d) config 4 asks for the
same decode on a DVB-S2-size code (N = 64800, K = 32400, E = 226799), which
only fits as a sparse matrix: this module builds such codes as CSR
(M, N, row_ptr, col_idx) for Decoder(csr=...) / ldpc_create_csr.

IRA codes in the DVB-S2 style (ETSI EN 302 307-1, 5.3.2): information bit m
of group g (360 bits per group) is checked by the rows (x + m*q) mod M for
every address x in row g of the code's address table, q = M / 360; the parity
part is the accumulator staircase (p_j = p_{j-1} ^ row j).  The ETSI tables
are not available offline, so dvbs2_like_table() draws a table with the
rate-1/2 normal frame's exact structure -- q = 90, 36 groups of degree 8 and
54 of degree 3, every residue mod q used 5 times, so every check row has
degree 7 (row 0: 6) and E = 226799 -- from a seed.  Results on it are
labelled "DVB-S2-like (synthetic address table)".

Column order: parity bits first (columns 0..M-1), information bits last
(M..N-1), matching the decoder's packed output (info = columns M..N-1, as
the reference's [parity; data] codewords, lib/ldpc_encoder_bc_impl.cc:153-165).
"""
import numpy as np

GROUP = 360


def dvbs2_like_table(seed=0, K=32400, N=64800, hi_groups=36, hi_deg=8, lo_deg=3):
    """Seeded address table with the DVB-S2 rate-1/2 normal-frame profile."""
    M = N - K
    q = M // GROUP
    groups = K // GROUP
    degs = [hi_deg] * hi_groups + [lo_deg] * (groups - hi_groups)
    total = sum(degs)
    if total % q:
        raise ValueError("degree profile does not spread evenly over the q residues")
    rng = np.random.Generator(np.random.PCG64(seed))
    residues = np.repeat(np.arange(q), total // q)
    rng.shuffle(residues)
    table, pos = [], 0
    for d in degs:
        row = set()
        for r in residues[pos:pos + d]:
            while True:
                x = int(r) + q * int(rng.integers(0, M // q))
                if x not in row:
                    row.add(x)
                    break
        table.append(sorted(row))
        pos += d
    return table


def ira_from_table(table, K, N):
    """CSR (M, N, row_ptr, col_idx) of the IRA code of an address table."""
    M = N - K
    if M % GROUP or K % GROUP or len(table) != K // GROUP:
        raise ValueError("K and N-K must be multiples of 360, one table row per 360 info bits")
    q = M // GROUP
    rows, cols = [], []
    m = np.arange(GROUP, dtype=np.int64)
    for g, addrs in enumerate(table):
        for x in addrs:
            rows.append((x + m * q) % M)
            cols.append(M + g * GROUP + m)
    # accumulator: row j holds parity bits j and j-1
    j = np.arange(M, dtype=np.int64)
    rows += [j, j[1:]]
    cols += [j, j[1:] - 1]
    r = np.concatenate(rows)
    c = np.concatenate(cols)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    if np.any((r[1:] == r[:-1]) & (c[1:] == c[:-1])):
        raise ValueError("address table places two ones in the same row and column")
    row_ptr = np.zeros(M + 1, np.int64)
    np.add.at(row_ptr, r + 1, 1)
    return M, N, np.cumsum(row_ptr).astype(np.int32), c.astype(np.int32)


def dvbs2_like(seed=0):
    """The config-4 code: N = 64800, K = 32400, E = 226799 (synthetic table)."""
    return ira_from_table(dvbs2_like_table(seed), 32400, 64800)


def ira_encode(csr, info_bits):
    """Systematic IRA encoding: (B, K) info bits -> (B, N) codewords
    [parity | info] with p_j = p_{j-1} ^ (info part of row j)."""
    M, N, row_ptr, col_idx = csr
    info = np.atleast_2d(np.asarray(info_bits, np.uint8)) & 1
    B = info.shape[0]
    # info part of each row = its ones at columns >= M
    rp = np.asarray(row_ptr, np.int64)
    ci = np.asarray(col_idx, np.int64)
    keep = ci >= M
    row_of = np.repeat(np.arange(M), np.diff(rp))[keep]
    s = np.zeros((B, M), np.uint8)
    vals = info[:, ci[keep] - M]
    for b in range(B):
        s[b] = np.bincount(row_of, weights=vals[b], minlength=M).astype(np.int64) & 1
    p = np.bitwise_xor.accumulate(s, axis=1)
    return np.concatenate([p, info], axis=1)


def syndrome_weight(csr, bits):
    """Unsatisfied checks of each (B, N) hard decision (checkFrame, uncapped)."""
    M, N, row_ptr, col_idx = csr
    bits = np.atleast_2d(np.asarray(bits, np.uint8)) & 1
    rp = np.asarray(row_ptr, np.int64)
    row_of = np.repeat(np.arange(M), np.diff(rp))
    out = np.zeros(bits.shape[0], np.int64)
    for b in range(bits.shape[0]):
        par = np.bincount(row_of, weights=bits[b, col_idx], minlength=M).astype(np.int64) & 1
        out[b] = par.sum()
    return out


# ---- quasi-cyclic codes ---------------------------------------------------------
#
# A base matrix of circulant shifts (mb, nb) and a lifting size Z (Decoder(qc=...),
# ldpc_create_qc): -1 is the zero block, s in [0, Z) the identity rotated by s.
# No standard base graph is available offline; qc_dual_diagonal() draws one with
# the dual-diagonal parity part of the 802.11n / 802.16e families from a seed.
# Results on it are labelled "QC dual-diagonal (synthetic base matrix)".
# qc_parity_core() draws the families' real parity shape (a weight-3 block
# column beside the dual diagonal, extension rows below), likewise synthetic.

def qc_expand(base, Z):
    """CSR (M, N, row_ptr, col_idx) of the code of base matrix `base` lifted by
    Z: row r*Z + i has a one in column c*Z + (i + s) mod Z for every entry
    base[r, c] = s >= 0."""
    base = np.asarray(base, np.int64)
    Z = int(Z)
    if base.ndim != 2 or Z < 1 or (base < -1).any() or (base >= Z).any():
        raise ValueError("base must be (mb, nb) with entries in [-1, Z)")
    mb, nb = base.shape
    br, bc = np.nonzero(base >= 0)
    i = np.arange(Z, dtype=np.int64)
    r = (br[:, None] * Z + i).reshape(-1)
    c = (bc[:, None] * Z + (i + base[br, bc][:, None]) % Z).reshape(-1)
    order = np.lexsort((c, r))
    row_ptr = np.zeros(mb * Z + 1, np.int64)
    np.add.at(row_ptr, r + 1, 1)
    return mb * Z, nb * Z, np.cumsum(row_ptr).astype(np.int32), c[order].astype(np.int32)


def qc_dual_diagonal(mb, nb, Z, info_deg, seed):
    """Seeded (mb, nb) base matrix: the parity part (block columns 0..mb-1) is
    the diagonal and the sub-diagonal at shift 0, and every information block
    column (mb..nb-1) has min(info_deg, mb) circulants in distinct block rows
    with shifts drawn from [0, Z)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    S = np.full((mb, nb), -1, np.int32)
    for r in range(mb):
        S[r, r] = 0
        if r >= 1:
            S[r, r - 1] = 0
    for c in range(mb, nb):
        rows = rng.choice(mb, size=min(info_deg, mb), replace=False)
        S[rows, c] = rng.integers(0, Z, size=rows.size)
    return S


def qc_parity_core(mc, me, nb, Z, info_deg, seed, a=1, b=0, x=None):
    """Seeded (mc + me, nb) base matrix with the parity part of the 802.11n /
    802.16e / 5G-NR families, which ldpc_encode_device and _capi.encode_qc
    encode: a core of mc block rows (0 for none, else >= 3) -- block column k,
    1 <= k < mc, holds shift 0 at (k-1, k) and (k, k); block column 0 holds
    shift a at (0, 0) and (mc-1, 0) and shift b at (x, 0), 0 < x < mc-1 (default
    mc // 2) -- and me extension rows, each with its diagonal entry at a drawn
    shift and up to two drawn entries left of it.  The information block
    columns (mc + me..nb-1) are drawn as qc_dual_diagonal draws them.  Results
    on it are labelled "QC parity-core (synthetic base matrix)"."""
    mb = mc + me
    if mc < 0 or mc in (1, 2) or me < 0 or mb < 1 or nb <= mb:
        raise ValueError("need mc = 0 or mc >= 3, me >= 0, mc + me >= 1 and nb > mc + me")
    rng = np.random.Generator(np.random.PCG64(seed))
    S = np.full((mb, nb), -1, np.int32)
    if mc:
        x = mc // 2 if x is None else int(x)
        if not (0 < x < mc - 1 and 0 <= a < Z and 0 <= b < Z):
            raise ValueError("need 0 < x < mc - 1 and a, b in [0, Z)")
        for k in range(1, mc):
            S[k - 1, k] = S[k, k] = 0
        S[0, 0] = S[mc - 1, 0] = a
        S[x, 0] = b
    for r in range(mc, mb):
        S[r, r] = rng.integers(0, Z)
        left = rng.choice(r, size=min(2, r), replace=False) if r else np.zeros(0, np.int64)
        S[r, left] = rng.integers(0, Z, size=left.size)
    for c in range(mb, nb):
        rows = rng.choice(mb, size=min(info_deg, mb), replace=False)
        S[rows, c] = rng.integers(0, Z, size=rows.size)
    return S


def qc_encode(csr, info_bits):
    """Systematic encoding of a code whose parity part (columns 0..M-1) is
    lower triangular with a unit diagonal, as qc_dual_diagonal's is: (B, K)
    info bits -> (B, N) codewords [parity | info], parity bit j, for j
    ascending, the mod-2 sum of the other columns of row j."""
    M, N, row_ptr, col_idx = csr
    info = np.atleast_2d(np.asarray(info_bits, np.uint8)) & 1
    cw = np.concatenate([np.zeros((info.shape[0], M), np.uint8), info], axis=1)
    for j in range(M):
        cols = np.asarray(col_idx[row_ptr[j]:row_ptr[j + 1]], np.int64)
        if not (cols == j).any() or ((cols < M) & (cols > j)).any():
            raise ValueError("row %d: the parity part is not lower triangular with a unit "
                             "diagonal" % j)
        cw[:, j] = np.bitwise_xor.reduce(cw[:, cols[cols != j]], axis=1) if cols.size > 1 else 0
    assert not syndrome_weight(csr, cw).any()
    return cw


def alist_text(H=None, csr=None, padded=True):
    """MacKay alist text of a dense H (M, N) or a CSR (M, N, row_ptr, col_idx):
    "N M", the maximum column / row degrees, the degrees, then each column's
    rows and each row's columns (1-based; zero-padded to the maximum degree
    when `padded`)."""
    if H is not None:
        H = np.asarray(H, np.uint8)
        M, N = H.shape
        rows = [np.nonzero(H[j])[0] for j in range(M)]
    else:
        M, N, rp, ci = csr
        rp = np.asarray(rp, np.int64)
        ci = np.asarray(ci, np.int64)
        rows = [np.sort(ci[rp[j]:rp[j + 1]]) for j in range(M)]
    cols = [[] for _ in range(N)]
    for j, r in enumerate(rows):
        for c in r:
            cols[int(c)].append(j)
    dv = [len(c) for c in cols]
    dc = [len(r) for r in rows]
    dvm, dcm = max(dv), max(dc)

    def line(v, width):
        v = [int(x) + 1 for x in v]
        if padded:
            v += [0] * (width - len(v))
        return " ".join(str(x) for x in v)
    out = ["%d %d" % (N, M), "%d %d" % (dvm, dcm), " ".join(map(str, dv)), " ".join(map(str, dc))]
    out += [line(c, dvm) for c in cols]
    out += [line(r, dcm) for r in rows]
    return "\n".join(out) + "\n"


def write_alist(path, H=None, csr=None, padded=True):
    with open(path, "w") as f:
        f.write(alist_text(H=H, csr=csr, padded=padded))


def read_alist(path):
    """(M, N, row_ptr, col_idx) of a MacKay alist file, read by the C ABI's
    ldpc_alist_read (include/ldpc_hip.h)."""
    from ._capi import alist_read
    return alist_read(path)
