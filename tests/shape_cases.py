"""Code shapes for every kernel variant the shape dispatch picks.

The decoder's hot paths are templates, and each context picks its
instantiations from the shape of its code: the small-code kernel from (NW,
low / generic loop lengths, column-centric or edge form, edge slots, row
slots), the large-code kernels from the degree bodies (check 8 / 16 / 32,
variable 4 / 8 / 16).  This module holds a deterministic code generator, a
table of named cases that reaches every such cell, the frames each case is
decoded on and the oracle's results for them (computed once per process).
tests/test_shape_cases.py checks on the CPU that the table covers the
dispatch; tests/test_gpu_shapes.py runs it on the device.

No code here has a column of degree > M / 2, so bit flipping (method 2) never
flips on this table: tests/bitflip_cases.py is the table for that.

When a dispatch cell is added (another slot count, loop length or degree
body), restate it in kernel_shape / graph_bodies below and add a case here:
the coverage test fails until the table reaches it."""
import os

import numpy as np

KEYS = ("bits", "packed", "iters", "synd")
B = 192          # frames per case
CAP = 20         # iteration cap
# Eb/N0 of frame b is EBN0[b % 6] dB.  A case whose oracle result lacks early
# or capped frames for one of methods 0-2 (tests/test_shape_cases.py checks
# each) gets a list of its own in the table, never a weaker assertion.
EBN0 = (0, 2, 4, 6, 8, 10)

# limits of the small-code kernel (csrc/ldpc_kernels.hpp)
K_DC_MAX, K_DV_MAX, K_SLOTS_MAX, K_N_MAX, K_M_MAX = 8, 4, 8, 256, 256


# ---- helpers shared by the GPU tests --------------------------------------------

def same_bits(a, b, what=""):
    """Posteriors as uint32 patterns: signed zeros and the sign and payload
    of NaNs count."""
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    bad = a != b
    assert not bad.any(), ("%s: %d of %d posteriors differ, first at %s: %s vs %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], [hex(v) for v in a[bad][:4]],
        [hex(v) for v in b[bad][:4]]))


def eq(out, ref, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %s" % (k, what))


def dense_to_csr(H):
    H = np.asarray(H, np.uint8)
    rows, cols = np.nonzero(H)
    rp = np.zeros(H.shape[0] + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32)


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ---- the dispatch, restated -------------------------------------------------------

def kernel_shape(M, N, E, dc, dv):
    """(slots, NW, DCN, DVN, cols) of the small-code kernel: the restatement
    of kernel_shape in csrc/ldpc_kernels.hpp, the one rule that the layout
    planner (csrc/ldpc_capi_create.hip) and the launchers' dispatch_small
    (csrc/ldpc_dispatch.hpp) both go by."""
    S = (E + 63) // 64
    NW = 1 if N <= 64 else 4
    low = NW == 1 and dc <= 6 and dv <= 3 and S <= 4
    dcn, dvn = (5, 3) if low else (K_DC_MAX - 1, K_DV_MAX)
    return S, NW, dcn, dvn, NW == 1 and dvn <= S


def fits_small(M, N, E, dc, dv):
    return (N <= K_N_MAX and M <= K_M_MAX and E <= 64 * K_SLOTS_MAX and dc <= K_DC_MAX and
            dv <= K_DV_MAX)


def graph_bodies(dc, dv):
    """(check body, variable body) of the large-code kernels
    (csrc/ldpc_graph.hip: g_check<PREC, DC>, g_var<Real, DV>, g_var_bf<DV>)."""
    return (8 if dc <= 8 else 16 if dc <= 16 else 32), (4 if dv <= 4 else 8 if dv <= 8 else 16)


def small_cells():
    """Every reachable (NW, generic, cols, slots) of the small-code kernel.
    NW = 1 holds N <= 64 columns of degree <= 4: at most 4 slots.  The low
    loop lengths need dv <= 3, so at most 3 slots, and are column-centric
    (DVN = 3 <= slots) at slots 3; the generic ones (DVN = 4) at slots 4.
    NW = 4 is never column-centric."""
    cells = set()
    for s in (1, 2, 3):
        cells.add((1, False, s >= 3, s))
    for s in (1, 2, 3, 4):
        cells.add((1, True, s >= 4, s))
    for s in range(1, 9):
        cells.add((4, True, False, s))
    return cells


# ---- the generator ------------------------------------------------------------------

def degree_vector(rng, N, counts):
    """N column degrees holding counts[d] columns of degree d, in a seeded order."""
    dv = np.concatenate([np.full(n, d, np.int64) for d, n in sorted(counts.items())])
    assert dv.size == N, (dv.size, N)
    return dv[rng.permutation(N)]


def random_code(M, N, dv):
    """H whose column i has dv[i] ones (dv: one degree for all columns, or
    {degree: columns}) in the rows of lowest degree so far, ties broken by
    the seeded generator: near-equal row degrees."""
    rng = np.random.Generator(np.random.PCG64(M * 1000 + N))
    if isinstance(dv, dict):
        dv = degree_vector(rng, N, dv)
    else:
        dv = np.full(N, dv, np.int64)
    H = np.zeros((M, N), np.uint8)
    deg = np.zeros(M)
    for i in range(N):
        rows = np.lexsort((rng.random(M), deg))[:dv[i]]
        H[rows, i] = 1
        deg[rows] += 1
    return H


def degree_limit_code():
    """M = 40, N = 120: a staircase (row 0 and column 38 of degree 1) plus
    random weight-3 columns, one column of degree 16 and one row filled up to
    degree 32.  Returns ((M, N, row_ptr, col_idx), H)."""
    M, N = 40, 120
    rng = np.random.Generator(np.random.PCG64(40))
    H = np.zeros((M, N), np.uint8)
    j = np.arange(M)
    H[j, j] = 1
    H[j[1:-1], j[1:-1] - 1] = 1      # row 39 keeps only its own column: column 38 has degree 1
    H[1:17, 40] = 1
    for c in range(41, N):
        H[rng.choice(np.arange(1, M), 3, replace=False), c] = 1
    free = [c for c in range(41, N) if not H[20, c]]
    for c in free[:32 - int(H[20].sum())]:
        H[20, c] = 1
    rp, ci = dense_to_csr(H)
    return (M, N, rp, ci), H


def _z_empty():
    H = random_code(16, 64, 2)
    H[:, 5] = 0
    H[3, :] = 0
    return H


# ---- the table ------------------------------------------------------------------------

class Case:
    """One code: `small` cases go through Decoder(H, reorder=False) onto the
    small-code kernel, the others through Decoder(csr=...) onto the large-code
    kernels.  expect: (E, dc_max, dv_max) the case is listed with, or None."""

    def __init__(self, name, small, make, expect=None, what="", ebn0=EBN0):
        self.name, self.small, self._make, self.expect, self.what = name, small, make, expect, what
        self.ebn0 = ebn0
        self._H = None
        self._frames = None
        self._refs = {}

    @property
    def H(self):
        if self._H is None:
            H = self._make()
            self._H = H[1] if isinstance(H, tuple) else H
            self._H.setflags(write=False)
        return self._H

    @property
    def csr(self):
        M, N = self.H.shape
        rp, ci = dense_to_csr(self.H)
        return M, N, rp, ci

    @property
    def shape(self):
        """dict: M, N, E, dc, dv, K, KB, rs and the dispatch cell."""
        H = self.H
        M, N = H.shape
        E, dc, dv = int(H.sum()), int(H.sum(1).max()), int(H.sum(0).max())
        d = dict(M=M, N=N, E=E, dc=dc, dv=dv, K=N - M, KB=(N - M + 7) // 8, rs=(M + 63) // 64,
                 bodies=graph_bodies(dc, dv))
        if self.small:
            S, NW, dcn, dvn, cols = kernel_shape(M, N, E, dc, dv)
            d.update(slots=S, NW=NW, generic=(dcn, dvn) != (5, 3), cols=cols)
        return d

    # frames and oracle results, once per process

    @property
    def frames(self):
        """The all-zero codeword, y = -1 + sigma * n, frame b at Eb/N0
        ebn0[b % 6] dB."""
        if self._frames is None:
            N = self.H.shape[1]
            rng = np.random.Generator(np.random.PCG64(5))
            db = np.asarray(self.ebn0, np.float64)[np.arange(B) % len(self.ebn0)]
            sigma = np.sqrt(10.0 ** (-db / 10))
            y = (-1.0 + sigma[:, None] * rng.standard_normal((B, N))).astype(np.float32)
            y.setflags(write=False)
            self._frames = y
        return self._frames

    def _oracle(self, method, y, cap=CAP, et=1):
        from oracle import oracle as orc
        ref = orc.decode_batch(method, self.H, y, cap, nthreads=threads(), want_post=True,
                               et_period=et)
        if not self.small:
            M, N, rp, ci = self.csr
            sp = orc.decode_batch_sparse(method, rp, ci, M, N, y, cap, nthreads=threads(),
                                         et_period=et)
            eq(ref, sp, what="%s method %d: dense vs sparse oracle" % (self.name, method))
        return ref

    def ref(self, method, cap=CAP, et=1):
        """The oracle's result on the case's frames (posteriors included)."""
        y = self.frames
        key = (method, cap, et)
        if key not in self._refs:
            self._refs[key] = self._oracle(method, y, cap, et)
        return self._refs[key]

    def ref_f32(self, cap=CAP, et=1):
        """The float oracle's min-sum on the case's frames (posteriors
        included): the contract of precision 1, method 0."""
        key = ("f32", cap, et)
        if key not in self._refs:
            from oracle import oracle as orc
            self._refs[key] = orc.decode_batch(0, self.H, self.frames, cap, nthreads=threads(),
                                               want_post=True, et_period=et, real="f32")
        return self._refs[key]

    def ref_for(self, tag, method, y, cap=CAP):
        """The oracle's result on other frames of this case, cached under tag."""
        key = (tag, method, cap)
        if key not in self._refs:
            self._refs[key] = self._oracle(method, y, cap)
        return self._refs[key]

    def counts(self, sparse=False):
        """{method: (early, capped)} frame counts of the oracle, methods 0-2
        (sparse: from its sparse restatement alone, which costs E rather
        than M * N per iteration)."""
        out = {}
        for m in (0, 1, 2):
            if sparse:
                from oracle import oracle as orc
                M, N, rp, ci = self.csr
                it = orc.decode_batch_sparse(m, rp, ci, M, N, self.frames, CAP, nthreads=threads(),
                                             want_bits=False)["iters"]
            else:
                it = self.ref(m)["iters"]
            out[m] = (int((it < CAP).sum()), int((it == CAP).sum()))
        return out


def early_and_capped(iters, cap=CAP):
    return bool((iters < cap).any() and (iters == cap).any())


def _rc(M, N, dv):
    return lambda: random_code(M, N, dv)


_CASES = [
    # the small-code kernel: name, M x N, column degrees, (E, dc_max, dv_max)
    Case("d_8x32", True, _rc(8, 32, 2), (64, 8, 2), "NW=1 generic, edge form, dc = 8"),
    Case("a_16x64", True, _rc(16, 64, 2), (128, 8, 2), "NW=1 generic, edge form, dc = 8"),
    Case("e_24x64", True, _rc(24, 64, 3), (192, 8, 3), "NW=1 generic, edge form"),
    Case("l_31x63", True, _rc(31, 63, {1: 10, 2: 20, 3: 17, 4: 16}), (165, 6, 4),
         "NW=1 generic, irregular, odd N, KB = 4"),
    Case("b_48x64", True, _rc(48, 64, 4), (256, 6, 4), "NW=1 generic, column-centric, DVN = 4, KB = 2"),
    Case("c_32x64", True, _rc(32, 64, 4), (256, 8, 4), "the same at dc = 8 and dv = 4, KB = 4"),
    Case("j_13x65", True, _rc(13, 65, {1: 36, 2: 29}), (94, 8, 2), "NW=4 at slots 2, dc 7-8, N = 65"),
    Case("i_24x96", True, _rc(24, 96, 2), (192, 8, 2), "NW=4 at slots 3, dc = 8, KB = 9"),
    Case("m_56x80", True, _rc(56, 80, 2), (160, 3, 2), "NW=4 with KB = 3: the window server's NW=4 build"),
    Case("k_37x101", True, _rc(37, 101, {1: 28, 2: 39, 3: 22, 4: 12}), (220, 6, 4),
         "NW=4 at slots 4, dv = 4, odd M and N"),
    Case("h_160x224", True, _rc(160, 224, 2), (448, 3, 2), "slots 7, rs = 3"),
    Case("g_250x256", True, _rc(250, 256, 2), (512, 3, 2), "rs = 4, KB = 1, every size at its limit"),
    Case("f_64x128", True, _rc(64, 128, 4), (512, 8, 4), "E = 512, dc = 8, dv = 4 together"),
    Case("z_empty", True, _z_empty, None, "a_16x64 with column 5 and row 3 cleared"),
    # the remaining cells: NW=4 at slots 1 (needs empty columns: 64 edges on more than
    # 64 columns), 5 and 6, and two row slots
    Case("n_12x70", True, _rc(12, 70, {0: 38, 2: 32}), (64, 6, 2), "NW=4 at slots 1: 38 empty columns"),
    Case("o_40x144", True, _rc(40, 144, 2), (288, 8, 2), "NW=4 at slots 5, dc 7-8"),
    Case("t_48x120", True, _rc(48, 120, 3), (360, 8, 3), "NW=4 at slots 6, dc 7-8"),
    Case("y_96x192", True, _rc(96, 192, 2), (384, 4, 2), "rs = 2"),
    # the large-code kernels
    Case("p_30x120", False, _rc(30, 120, 3), (360, 12, 3), "g_check<16>"),
    Case("q_60x150", False, _rc(60, 150, {1: 25, 2: 25, 3: 25, 4: 20, 5: 20, 6: 15, 7: 10, 8: 10}),
         (570, 10, 8), "g_check<16>, g_var<8>, g_var_bf<8>, irregular degrees"),
    Case("r_40x300", False, _rc(40, 300, 4), (1200, 30, 4), "g_check<32>, KB = 33"),
    Case("s_48x96", False, _rc(48, 96, {3: 88, 13: 8}), (368, 8, 13), "g_var<16>, g_var_bf<16>"),
    Case("limit_40x120", False, degree_limit_code, (None, 32, 16), "dc 32 and dv 16: both limits"),
    # the remaining body pairs
    Case("u_48x96", False, _rc(48, 96, {3: 88, 6: 8}), (312, 7, 6), "check body 8 with variable body 8"),
    Case("v_30x120", False, _rc(30, 120, {3: 116, 13: 4}), (400, 14, 13), "check body 16 with variable body 16"),
    Case("w_40x300", False, _rc(40, 300, {4: 290, 6: 10}), (1220, 31, 6), "check body 32 with variable body 8"),
]
CASES = {c.name: c for c in _CASES}
SMALL = [c.name for c in _CASES if c.small]
LARGE = [c.name for c in _CASES if not c.small]
