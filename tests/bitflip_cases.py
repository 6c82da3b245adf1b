"""Codes on which bit flipping really flips, and the frames they are decoded on.

decodeBitFlipping (lib/ldpc_decoder_cb_impl.cc:414-476) flips column j only
when more than M / 2 of its checks disagree with the channel decision, so
only a column of degree > M / 2 can ever flip.  No code of
tests/shape_cases.py, no golden frame and no standard code has one: there
method 2 equals method 3 and stops at iteration 1 or at the cap.  The codes
here have few rows and heavy columns.  A table of its own, because the shape
table wants early and capped frames of methods 0 and 1 too and runs every
entry point for every method; Case, the helpers and the restated dispatch
are shape_cases'.

Frames of a case (FRAMES of them, not a multiple of 64, so the large-code
path's last chunk is partial), all on the all-zero codeword:
  noise      y = -1 + sigma * n at 0..10 dB, as in shape_cases
  sign       magnitudes in [0.25, 1.25], 1..wmax sign errors on columns that
             have checks (sign_pool, seeded)
  found      frames of the same pool that a seeded search found to stop at
             1 < iters < CAP; they sit inside the first 64-frame chunk, next
             to frames that stop at 1 and at the cap
  solved     in their place on g_31x62, where no such frame can exist: sign
             patterns with a chosen syndrome (solved_frames)
tests/test_bitflip_ref_host.py asserts what the frames must show (flips,
changes after iteration 1, intermediate stops, every mutant of
tests/bitflip_ref.py told apart) and that the table reaches both
launch_hard instantiations and the three g_var_bf bodies;
tests/test_gpu_bitflip.py runs it on the device.

The search (profiles/round26/bitflip.txt has its extent and counts): per
shape, code seeds 0..299, each with its 768-frame sign pool, decoded by
bitflip_ref at the cap of 20; the seed with the most intermediate stops whose
frames also meet every condition of the host test was taken."""
import numpy as np

from shape_cases import CAP, EBN0, Case

FRAMES, N_NOISE, POOL = 200, 96, 768
FOUND_AT = 16        # the found frames start here: inside the first 64-frame chunk


def flip_code(M, N, dv, seed):
    """shape_cases.random_code with a seed of its own: column i gets dv[i]
    ones (dv: one degree, {degree: columns} in a seeded order, or a degree
    per column) in the rows of lowest degree so far, ties broken at random."""
    rng = np.random.Generator(np.random.PCG64([M, N, seed]))
    if isinstance(dv, dict):
        d = np.concatenate([np.full(n, k, np.int64) for k, n in sorted(dv.items())])
        assert d.size == N, (d.size, N)
        d = d[rng.permutation(N)]
    else:
        d = np.broadcast_to(np.asarray(dv, np.int64), (N,))
    H = np.zeros((M, N), np.uint8)
    deg = np.zeros(M)
    for i in range(N):
        rows = np.lexsort((rng.random(M), deg))[:d[i]]
        H[rows, i] = 1
        deg[rows] += 1
    return H


def noise_frames(N, n=N_NOISE, ebn0=EBN0):
    """shape_cases' frames: y = -1 + sigma * n, frame b at ebn0[b % 6] dB."""
    rng = np.random.Generator(np.random.PCG64(5))
    db = np.asarray(ebn0, np.float64)[np.arange(n) % len(ebn0)]
    sigma = np.sqrt(10.0 ** (-db / 10))
    return (-1.0 + sigma[:, None] * rng.standard_normal((n, N))).astype(np.float32)


def sign_pool(H, seed, n=POOL, wmax=4):
    """n frames of magnitudes in [0.25, 1.25], all negative (the all-zero
    codeword) but for 1 + b % wmax sign errors on columns that have checks."""
    N = H.shape[1]
    rng = np.random.Generator(np.random.PCG64([N, seed, 77]))
    y = -(0.25 + rng.random((n, N))).astype(np.float32)
    cols = np.flatnonzero(H.sum(0) > 0)
    for b in range(n):
        e = rng.choice(cols, size=min(1 + b % wmax, cols.size), replace=False)
        y[b, e] = -y[b, e]
    return y


def solved_frames(H, seed):
    """Eight sign patterns with a chosen syndrome, for a code whose columns
    flip only when all their checks are unsatisfied (degree M / 2 + 1) and so
    hardly ever flip two at a time on seeded patterns.  H e = s is solved
    over GF(2), the free columns seeded: s = all ones (every column of full
    degree flips at once), s = the rows of column j plus one other row (j
    flips, one check stays unsatisfied, and j collects all its votes again in
    every later iteration), s = the rows of columns j and k (both flip, and
    each then sees the other's flip in the checks they share)."""
    from gf2_ref import eliminate
    M, N = H.shape
    rng = np.random.Generator(np.random.PCG64([N, seed, 99]))
    heavy = np.flatnonzero(H.sum(0) > M // 2)
    targets = [np.ones(M, np.uint8)] * 2
    for j in heavy[[0, -1, len(heavy) // 2]]:
        s = H[:, j].copy()
        s[rng.choice(np.flatnonzero(s == 0))] = 1
        targets.append(s)
    for j, k in ((heavy[0], heavy[1]), (heavy[-1], heavy[-2]), (heavy[2], heavy[-3])):
        targets.append(H[:, j] | H[:, k])
    S = np.stack(targets).T                                         # (M, 8)
    A, piv = eliminate(np.concatenate([H, S], axis=1), N)
    assert len(piv) == M, "H has dependent rows: a syndrome may have no sign pattern"
    free = np.setdiff1d(np.arange(N), piv)
    e = np.zeros((len(targets), N), np.uint8)
    e[:, free] = rng.integers(0, 2, size=(len(targets), free.size))
    e[:, piv] = (A[:, N:].T + e[:, free].astype(np.int64) @ A[:, free].T.astype(np.int64)) % 2
    assert (((e.astype(np.int64) @ H.T.astype(np.int64)) % 2) == S.T).all()
    mag = (0.25 + rng.random(e.shape)).astype(np.float32)
    return np.where(e == 1, mag, -mag).astype(np.float32)


class FlipCase(Case):
    """A Case whose code comes from flip_code(M, N, dv, seed) and whose
    frames are noise, sign and found frames (module docstring).  found:
    indices into the case's sign pool, or "solved": solved_frames in their
    place."""

    def __init__(self, name, small, M, N, dv, seed, expect, found, what, wmax=4):
        Case.__init__(self, name, small, lambda: flip_code(M, N, dv, seed), expect, what)
        self.solved = found == "solved"
        self.seed, self.found, self.wmax = seed, () if self.solved else tuple(found), wmax
        self.odd = M % 2 == 1

    @property
    def frames(self):
        if self._frames is None:
            noise = noise_frames(self.H.shape[1])
            pool = sign_pool(self.H, self.seed, wmax=self.wmax)
            extra = solved_frames(self.H, self.seed) if self.solved else pool[list(self.found)]
            n_sign = FRAMES - N_NOISE - len(extra)
            y = np.concatenate([noise[:FOUND_AT], extra, noise[FOUND_AT:],
                                pool[:n_sign]]).astype(np.float32)
            assert y.shape[0] == FRAMES and FRAMES % 64 != 0
            y.setflags(write=False)
            self._frames = y
        return self._frames

    @property
    def can_flip(self):
        """Columns of degree > M / 2: the only ones the vote can ever flip."""
        return self.H.sum(0) > self.H.shape[0] // 2

    def special_frames(self):
        """The case's frames with +-0.0, NaN and +-inf on strides of frames, at
        columns that can flip: y = !(rx < 0), so +-0.0 and NaN decide 1."""
        y = np.array(self.frames)
        c = np.flatnonzero(self.can_flip)
        y[0::3, c[0]] = 0.0
        y[1::3, c[-1]] = -0.0
        y[2::5, c[len(c) // 2]] = 0.0
        y[3::7, c[len(c) // 3]] = np.nan
        y[4::9, c[1]] = np.inf
        y[5::11, c[-2]] = -np.inf
        return y


def early_mid_capped(iters, cap=CAP):
    """Frames that stop at 1, at an intermediate count and at the cap."""
    return bool((iters == 1).any() and ((iters > 1) & (iters < cap)).any() and (iters == cap).any())


_ALT = [10, 11] * 14 + [16] * 12     # h_20x40: degrees M / 2 and M / 2 + 1 side by side
# NW = 4 by empty columns in the middle: columns that can flip in both 64-column words
_C70 = [4, 2, 3, 1, 2, 3, 2] + [0] * 56 + [2, 4, 1, 3, 2, 1, 4]
_D70 = [4, 2, 3, 1, 3, 2] + [0] * 58 + [3, 4, 1, 2, 3, 4]
# one column of degree 15 = M / 2, which cannot flip: with 16 everywhere every column has
# even weight, H loses a rank and only syndromes of even weight have a sign pattern
_G62 = [16] * 30 + [15] + [16] * 31

# name, small, M, N, column degrees, code seed, (E, dc_max, dv_max), found frames, what.
# `found` empty: the search (module docstring) found no frame with 1 < iters < CAP.
#   b_4x12, d_4x70: none in 300 seeds x 768 frames; M = 4 is the only even M a small code
#     can have with a column of degree > M / 2 + 1 (dv <= 4).
#   g_31x62: none can exist.  dv_max = 16 = M / 2 + 1, so a column flips only when all
#     its checks are unsatisfied.  A column that does not flip at iteration 1 has a
#     satisfied check; no member of a satisfied check flips, so that check, and with it
#     the column, stays as it is for ever: the decision never changes after iteration 1
#     (the host test asserts this), and a frame stops at 1 or at the cap.  On seeded
#     patterns two of its columns hardly ever flip in one frame, which the mutants that
#     show only after iteration 1 need: it gets solved_frames in place of found ones.
_CASES = [
    # the small-code kernel, launch_hard<1>: N <= 64
    FlipCase("a_5x14", True, 5, 14, {1: 3, 2: 5, 3: 3, 4: 3}, 265, (34, 7, 4),
             (3, 6, 18, 20, 27, 29, 32, 36), "NW=1, odd M, only degrees 3 and 4 can flip"),
    FlipCase("b_4x12", True, 4, 12, {1: 2, 2: 3, 3: 4, 4: 3}, 0, (32, 8, 4), (),
             "NW=1, even M, dc = 8, only degrees 3 and 4 can flip"),
    # launch_hard<4>: N > 64, by empty columns
    FlipCase("c_5x70", True, 5, 70, _C70, 67, (34, 7, 4), (27, 39, 40, 68, 87, 95, 100, 126),
             "NW=4, odd M: a_5x14's degrees, 56 empty columns between columns 6 and 63"),
    FlipCase("d_4x70", True, 4, 70, _D70, 0, (32, 8, 4), (),
             "NW=4, even M: b_4x12's degrees, 58 empty columns, the last six in the second word"),
    # g_var_bf<8>: dv 5..8, so M <= 15
    FlipCase("e_11x40", False, 11, 40, {3: 10, 5: 10, 6: 8, 7: 6, 8: 6}, 78, (218, 20, 8),
             (284, 360, 428, 488, 548, 572, 720, 77), "g_var_bf<8>, odd M, degrees 6..8 can flip"),
    FlipCase("f_12x40", False, 12, 40, {3: 8, 5: 6, 6: 8, 7: 10, 8: 8}, 238, (236, 20, 8),
             (489, 721, 751), "g_var_bf<8>, even M, degree 6 = M / 2 cannot flip, 7 can"),
    # g_var_bf<16>: dv 9..16, so M <= 31
    FlipCase("g_31x62", False, 31, 62, _G62, 0, (991, 32, 16), "solved",
             "g_var_bf<16>, M = 31 with dv = 16 and dc = 32: every limit at once"),
    FlipCase("h_20x40", False, 20, 40, _ALT, 114, (486, 25, 16), (7,),
             "g_var_bf<16>, even M, degrees 10 = M / 2 and 11 side by side", wmax=8),
    FlipCase("i_21x42", False, 21, 42, {11: 14, 12: 8, 14: 10, 16: 10}, 251, (550, 27, 16), (514,),
             "g_var_bf<16>, odd M, every column can flip", wmax=8),
]
CASES = {c.name: c for c in _CASES}
SMALL = [c.name for c in _CASES if c.small]      # also g_var_bf<4>: force_graph, Decoder(csr=...)
LARGE = [c.name for c in _CASES if not c.small]
NO_LATER = ("g_31x62",)                          # proved above: nothing changes after iteration 1

