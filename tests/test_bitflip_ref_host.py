"""Bit flipping on codes where a bit really flips: the references, host only.

decodeBitFlipping (lib/ldpc_decoder_cb_impl.cc:414-476) can flip only a
column of degree > M / 2, which no other code of the suite has, so there the
oracle's three restatements agree trivially (none of them ever flips).  Here:
tests/bitflip_ref.py, a fourth restatement written from the text, is pinned
to an example worked by hand; the four agree on every code of
tests/bitflip_cases.py; the cases' frames show what they are there to show
(flips, changes after iteration 1, stops at intermediate counts); every
mutant of bitflip_ref is told apart by every case; and the table reaches
both launch_hard instantiations and the three g_var_bf bodies.  Run with -s
to see the counts (profiles/round26/bitflip.txt keeps them)."""
import os
import re

import numpy as np
import pytest

import bitflip_cases as bc
import bitflip_ref as bfr
from bitflip_cases import CASES, LARGE, NO_LATER, SMALL
from shape_cases import CAP, early_and_capped, fits_small, graph_bodies, kernel_shape, threads

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "gr-ldpc_ece535a_amd", "csrc")
ALL = SMALL + LARGE
CAPS, ETS = (1, 2, 20), (1, 5)


def differs(a, b):
    return any((a[k] != b[k]).any() for k in ("bits", "iters", "synd"))


# ---- 1. worked by hand ---------------------------------------------------------------------

def test_hand_worked_example():
    """M = 4, so M / 2 = 2 and a column needs 3 disagreeing checks to flip.

        columns  0 1 2 3 4 5        rows of column 0: 0 1 2     3: 0 1
        row 0    1 . 1 1 . 1                        1: 1 2 3     4: 2 3
        row 1    1 1 . 1 . 1                        2: 0 3       5: 0 1 2 3
        row 2    1 1 . . 1 1
        row 3    . 1 1 . 1 1

    The all-zero codeword with a sign error on column 0: y = 1 0 0 0 0 0.
    E(i, j) of an edge is the parity of the row's other columns, (row parity)
    ^ ci(j); a vote is an edge with E(i, j) != y(j).

    Iteration 1, ci = y, row parities 1 1 1 0:
      column 0 (y 1): E = 0 0 0, 3 votes > 2: becomes 1 - y = 0
      column 1 (y 0): E = 1 1 0, 2 votes: not more than 2, stays (">=" flips it)
      column 2: E = 1 0, 1 vote.  column 3: E = 1 1, 2 votes.  column 4: E = 1 0, 1 vote
      column 5 (y 0): E = 1 1 1 0, 3 votes: becomes 1, wrongly
      ci = 0 0 0 0 0 1, every row unsatisfied: weight 4
    Iteration 2, all votes from that ci, row parities 1 1 1 1:
      column 0 (y 1, ci 0): E = 1 1 1 = y, no vote: stays 0, it does not fall back to y
      column 1 (y 0): E = 1 1 1, 3 votes: becomes 1
      columns 2, 3, 4: 2 votes each (degree 2).  column 5 (ci 1): E = 0 0 0 0: stays 1
      ci = 0 1 0 0 0 1, row parities 1 0 0 0: weight 1
    Iteration 3:
      column 0 (y 1, ci 0): E = 1 0 0, 2 votes: stays
      column 1 (y 0, ci 1): E = 1 1 1, 3 votes: 1 - y = 1 again (a toggle would give 0)
      column 5 (y 0, ci 1): E = 0 1 1 1, 3 votes: 1 again.  columns 2, 3, 4: at most 1 vote
      ci unchanged, and so for every later iteration: the cap is reached."""
    H = np.array([[1, 0, 1, 1, 0, 1],
                  [1, 1, 0, 1, 0, 1],
                  [1, 1, 0, 0, 1, 1],
                  [0, 1, 1, 0, 1, 1]], np.uint8)
    rx = np.array([[0.5, -1, -1, -1, -1, -1]], np.float32)
    want = {1: ([0, 0, 0, 0, 0, 1], 4), 2: ([0, 1, 0, 0, 0, 1], 1), 3: ([0, 1, 0, 0, 0, 1], 1),
            9: ([0, 1, 0, 0, 0, 1], 1)}
    for cap, (bits, synd) in want.items():
        out = bfr.decode(H, rx, cap)
        assert out["bits"][0].tolist() == bits and out["synd"][0] == synd, (cap, out)
        assert out["iters"][0] == cap
    # the wrong readings this example alone tells apart
    assert bfr.decode(H, rx, 1, mutant="ge")["bits"][0].tolist() == [0, 1, 0, 1, 0, 1]
    assert bfr.decode(H, rx, 2, mutant="reset")["bits"][0, 0] == 1
    assert bfr.decode(H, rx, 3, mutant="toggle")["bits"][0, 1] == 0
    # a sign error on column 2, which cannot flip: its rows 0 and 3 are unsatisfied, no
    # column collects 3 votes, nothing ever changes
    rx = np.array([[-1, -1, 0.5, -1, -1, -1]], np.float32)
    out = bfr.decode(H, rx, 7)
    assert out["bits"][0].tolist() == [0, 0, 1, 0, 0, 0] and out["synd"][0] == 2 and out["iters"][0] == 7
    # the noise-free frame stops after one iteration; with a cap of 1 it is counted as capped
    out = bfr.decode(H, -np.ones((1, 6), np.float32), 7)
    assert not out["bits"].any() and out["iters"][0] == 1 and out["synd"][0] == 0


def test_hard_decision_of_special_samples():
    """y = !(rx < 0): 0 only for negative samples, -inf included; +-0.0 and
    NaN decide 1 (:424-431), under either polarity for the zeros."""
    rx = np.array([[-1.0, 1.0, 0.0, -0.0, np.nan, np.inf, -np.inf]], np.float32)
    assert bfr.hard(rx)[0].tolist() == [0, 1, 1, 1, 1, 1, 0]
    assert bfr.hard(rx, polarity=-1.0)[0].tolist() == [1, 0, 1, 1, 1, 0, 1]


# ---- 2. the four restatements ---------------------------------------------------------------

def python_oracle(H, y, cap, et):
    from oracle import ldpc_oracle_py as opy
    Hl = [[int(v) for v in row] for row in H]
    bits = np.zeros(y.shape, np.uint8)
    iters = np.zeros(y.shape[0], np.int32)
    for b in range(y.shape[0]):
        v, used = opy.decode(2, Hl, [float(x) for x in y[b]], cap, et)
        bits[b], iters[b] = v, used
    synd = ((bits.astype(np.int64) @ np.asarray(H, np.int64).T) % 2).sum(1).astype(np.int32)
    return dict(bits=bits, iters=iters, synd=synd)


@pytest.mark.parametrize("name", ALL)
def test_four_restatements_agree(name):
    """The dense and the sparse C oracle, ldpc_oracle_py and bitflip_ref:
    bits, iterations and syndrome weights at caps 1, 2 and 20 and et_period 1
    and 5; also on the special samples and under the opposite polarity."""
    from oracle import oracle as orc
    c = CASES[name]
    M, N, rp, ci = c.csr
    for y, tag in ((c.frames, "frames"), (c.special_frames(), "special samples")):
        for cap in CAPS:
            for et in ETS:
                what = "%s %s cap %d et_period %d" % (name, tag, cap, et)
                ref = bfr.decode(c.H, y, cap, et)
                dense = orc.decode_batch(2, c.H, y, cap, nthreads=threads(), et_period=et)
                sparse = orc.decode_batch_sparse(2, rp, ci, M, N, y, cap, nthreads=threads(),
                                                 et_period=et)
                for other, who in ((dense, "dense C"), (sparse, "sparse C")):
                    for k in ("bits", "iters", "synd"):
                        np.testing.assert_array_equal(other[k], ref[k], err_msg="%s: %s %s" % (
                            what, who, k))
                np.testing.assert_array_equal(dense["packed"], sparse["packed"], err_msg=what)
                if tag == "frames":
                    # interpreted, dc^2 steps per row: at the cap of 20 the body-16 codes get
                    # the first chunk (found or solved frames included) and every 4th frame
                    pick = np.arange(y.shape[0])
                    if cap == CAP and c.shape["dv"] > 8:
                        pick = np.concatenate([pick[:64], pick[64::4]])
                    py = python_oracle(c.H, y[pick], cap, et)
                    for k in ("bits", "iters", "synd"):
                        np.testing.assert_array_equal(py[k], ref[k][pick], err_msg=(
                            "%s: python %s" % (what, k)))
    neg = bfr.decode(c.H, c.frames, CAP, polarity=-1.0)
    dense = orc.decode_batch(2, c.H, c.frames, CAP, polarity=-1.0, nthreads=threads())
    for k in ("bits", "iters", "synd"):
        np.testing.assert_array_equal(dense[k], neg[k], err_msg="%s polarity -1 %s" % (name, k))
    assert differs(neg, bfr.decode(c.H, -np.array(c.frames), CAP)) is False


# ---- 3. what the frames must show --------------------------------------------------------------

def observed(c):
    """Counts over the case's frames, from bitflip_ref."""
    y = c.frames
    r20, r1 = bfr.decode(c.H, y, CAP), bfr.decode(c.H, y, 1)
    it = r20["iters"]
    return dict(flipped=int((r20["bits"] != bfr.hard(y)).any(1).sum()),
                later=int((r20["bits"] != r1["bits"]).any(1).sum()),
                unflippable=int((r20["bits"] != bfr.hard(y))[:, ~c.can_flip].sum()),
                iters={int(v): int((it == v).sum()) for v in np.unique(it)}, it=it)


@pytest.mark.parametrize("name", ALL)
def test_frames_show_what_they_are_for(name):
    c = CASES[name]
    s = c.shape
    assert c.small == fits_small(s["M"], s["N"], s["E"], s["dc"], s["dv"]), (name, s)
    assert c.expect == (s["E"], s["dc"], s["dv"]), (name, s)
    assert c.frames.shape == (bc.FRAMES, s["N"]) and bc.FRAMES % 64 != 0
    assert c.can_flip.any() and s["dv"] > s["M"] // 2
    o = observed(c)
    it = o.pop("it")
    print("\n%s: %s" % (name, o))
    # method 2 differs from method 3, and only on columns of degree > M / 2
    assert o["flipped"] > 0 and o["unflippable"] == 0, (name, o)
    # the oracle's own method 3 is the control the GPU test uses
    assert (c.ref(3)["bits"] == bfr.hard(c.frames)).all()
    assert early_and_capped(it), (name, o)
    if name in NO_LATER:
        # dv_max = M / 2 + 1: proved in bitflip_cases that nothing changes after iteration 1
        assert o["later"] == 0 and set(o["iters"]) == {1, CAP}, (name, o)
    else:
        assert o["later"] > 0, (name, o)
    if c.solved:
        # the solved frames: every column that can flip at once (twice), one column, two
        # columns or more (neighbouring columns take complementary rows: their union is all)
        n = (c.ref(2)["bits"] != bfr.hard(c.frames))[bc.FOUND_AT:bc.FOUND_AT + 8].sum(1)
        assert n[:5].tolist() == [int(c.can_flip.sum())] * 2 + [1] * 3 and (n[5:] >= 2).all(), (name, n)
    if c.found:
        assert bc.early_mid_capped(it), (name, o)
        assert bc.early_mid_capped(it[:64]), "%s: not within one 64-frame chunk" % name
        found = it[bc.FOUND_AT:bc.FOUND_AT + len(c.found)]
        assert ((found > 1) & (found < CAP)).all(), (name, found)
    # et_period 5: some frame would have stopped earlier at et_period 1
    it5 = bfr.decode(c.H, c.frames, CAP, 5)["iters"]
    assert (it5 % 5 == 0).all() and (it5 > it).any(), name


def test_every_kernel_family_has_an_intermediate_stop():
    """NW = 1, NW = 4 (and with them body 4), body 8 and body 16 each have a
    frame with 1 < iters < cap; body 16 only on sign patterns of weight up to
    8 (h_20x40, i_21x42)."""
    groups = {}
    for name in ALL:
        c = CASES[name]
        key = "NW%d" % c.shape["NW"] if c.small else "body%d" % c.shape["bodies"][1]
        groups.setdefault(key, []).append(bool(c.found))
    assert set(groups) == {"NW1", "NW4", "body8", "body16"} and all(any(v) for v in groups.values())


# ---- 4. mutants ----------------------------------------------------------------------------------

def kills(c):
    """{mutant: (cap, et_period) settings at which it changes bits, iters or
    synd on the case's frames}.  le0 runs on the special samples."""
    out = {}
    for m in bfr.MUTANTS:
        y = c.special_frames() if m == "le0" else c.frames
        out[m] = [(cap, et) for cap in CAPS for et in ETS
                  if differs(bfr.decode(c.H, y, cap, et), bfr.decode(c.H, y, cap, et, mutant=m))]
    return out


@pytest.mark.parametrize("name", ALL)
def test_every_mutant_changes_the_result(name):
    c = CASES[name]
    k = kills(c)
    print("\n%s: %s" % (name, {m: len(v) for m, v in k.items()}))
    for m, where in k.items():
        if m == "ceil" and not c.odd:
            assert not where, (name, m)       # (M + 1) / 2 == M / 2
        elif m == "no_et":
            assert where and all(et == 5 for _, et in where), (name, m, where)
        elif m == "late_bound":
            assert (2, 1) in where, (name, m, where)   # a stop at iteration 1 = cap - 1
        else:
            assert (CAP, 1) in where, (name, m, where)
    # an exit allowed at the last iteration is the same decoder: the loop ends there anyway
    for cap in CAPS:
        assert not differs(bfr.decode(c.H, c.frames, cap), bfr.decode(c.H, c.frames, cap,
                                                                      mutant="last_exit"))


# ---- 5. coverage -----------------------------------------------------------------------------------

def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_table_reaches_every_bit_flip_kernel():
    """Read from the sources: launch_hard<NW> for NW 1 and 4, g_var_bf<DV> for
    DV 4, 8 and 16 at dv_max <= 4, <= 8 and above.  Every such kernel has an
    odd-M and an even-M case whose decision changes after iteration 1, and
    body 16 has the case at every limit and the one with degrees M / 2 and
    M / 2 + 1 side by side: a case removed from the table fails here."""
    k = source("ldpc_kernels.hip")
    nws = sorted(int(v) for v in re.findall(r"launch_hard<(\d)>\(code, a, method, st\)", k))
    assert nws == [1, 4]
    assert "nw == 1 ? launch_hard<1>(code, a, method, st) : nw == 4 ? launch_hard<4>" in k
    g = source("ldpc_graph.hip")
    assert re.findall(r"g_var_bf<(\d+)><<<", g) == ["4", "8", "16"]
    assert re.search(r"if \(g\.dv_max <= 4\)\s+g_var_bf<4><<<", g)
    assert re.search(r"else if \(g\.dv_max <= 8\)\s+g_var_bf<8><<<", g)
    assert graph_bodies(8, 4)[1] == 4 and graph_bodies(8, 5)[1] == 8 and graph_bodies(8, 9)[1] == 16
    want = {(kern, odd) for kern in [("launch_hard", n) for n in nws] +
            [("g_var_bf", 4), ("g_var_bf", 8), ("g_var_bf", 16)] for odd in (False, True)}
    reached = {}
    for name in ALL:
        c = CASES[name]
        if name in NO_LATER:
            continue
        s = c.shape
        if c.small:
            S, NW, dcn, dvn, cols = kernel_shape(s["M"], s["N"], s["E"], s["dc"], s["dv"])
            assert NW == s["NW"]
            reached.setdefault((("launch_hard", NW), c.odd), []).append(name)
        # the small cases reach g_var_bf<4> by force_graph and by Decoder(csr=...)
        reached.setdefault((("g_var_bf", s["bodies"][1]), c.odd), []).append(name)
    assert set(reached) == want, sorted(want ^ set(reached))
    # ... each by one case only (body 4 by one per NW): none is redundant
    assert all(len(v) == (2 if k[0] == ("g_var_bf", 4) else 1) for k, v in reached.items()), reached
    assert sorted(n for v in reached.values() for n in v if n in LARGE) + list(NO_LATER) == sorted(
        LARGE, key=lambda n: (n in NO_LATER, n))
    lim = CASES["g_31x62"].shape
    assert (lim["M"], lim["dv"], lim["dc"]) == (31, 16, 32)
    assert sorted(CASES["g_31x62"].H.sum(0))[:2] == [15, 16]     # M / 2 next to M / 2 + 1
    d = CASES["h_20x40"].H.sum(0)
    half = CASES["h_20x40"].H.shape[0] // 2
    assert any(d[j] == half and d[j + 1] == half + 1 for j in range(d.size - 1))
    assert not CASES["h_20x40"].can_flip[d == half].any() and CASES["h_20x40"].can_flip[d == half + 1].all()
    # mixed degrees on the small-code kernel: only some columns can flip
    for name in ("a_5x14", "b_4x12", "c_5x70", "d_4x70"):
        f = CASES[name].can_flip
        assert f.any() and not f[CASES[name].H.sum(0) > 0].all(), name
    for name in ("c_5x70", "d_4x70"):   # both words of an NW = 4 frame hold columns that can flip
        f = np.flatnonzero(CASES[name].can_flip)
        assert (f < 64).any() and (f >= 64).any(), (name, f)


if __name__ == "__main__":   # the record kept in profiles/round26/bitflip.txt
    print("per case: shape, frames of %d whose method-2 bits differ from method 3 (flipped), whose\n"
          "cap-20 bits differ from cap-1 bits (later), iteration histogram at the cap of %d, and per\n"
          "mutant the (cap, et_period) settings of %s x %s at which it changes bits, iterations or\n"
          "syndromes (le0 on the special samples)" % (bc.FRAMES, CAP, CAPS, ETS))
    for case in bc._CASES:
        o = observed(case)
        o.pop("it")
        sh = case.shape
        print("\n%s  M %d N %d E %d dc %d dv %d  columns that can flip %d  (%s)" % (
            case.name, sh["M"], sh["N"], sh["E"], sh["dc"], sh["dv"], case.can_flip.sum(), case.what))
        print("  flipped %d  later %d  iters %s" % (o["flipped"], o["later"], o["iters"]))
        for m, where in kills(case).items():
            print("  %-10s %s" % (m, where if where else "-  (same decoder for even M)"))
