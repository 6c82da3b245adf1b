"""The shape table (tests/shape_cases.py) reaches every kernel variant the
shape dispatch can pick.  Host only: the dispatch rule is restated in
shape_cases.kernel_shape / graph_bodies, the restatement is held against the
dispatch sources (so a cell added there fails here until the table has a
case for it), and the table is held against the restatement.  Also: every
case has the shape it is listed with, takes the path it is meant for, and
its frames give the oracle both early and capped frames for methods 0-2."""
import os
import re

import numpy as np
import pytest

import shape_cases as sc
from shape_cases import CASES, LARGE, SMALL

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "gr-ldpc_ece535a_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_restated_limits_match_the_headers():
    hpp = source("ldpc_kernels.hpp")
    assert (sc.K_DC_MAX, sc.K_DV_MAX, sc.K_SLOTS_MAX, sc.K_N_MAX, sc.K_M_MAX) == tuple(
        constant(hpp, n) for n in ("kDcMax", "kDvMax", "kSlotsMax", "kNMax", "kMMax"))
    g = source("ldpc_graph.hpp")
    assert (constant(g, "kGraphDcMax"), constant(g, "kGraphDvMax")) == (32, 16)


def test_restated_dispatch_matches_the_sources():
    """The instantiations the dispatch code names are the cells restated in
    shape_cases: slot counts 1..8 with the generic loops, 1..4 with the low
    ones (dc <= 6, dv <= 3, NW = 1), NW 1 and 4, check bodies 8 / 16 / 32 and
    variable bodies 4 / 8 / 16."""
    k = source("ldpc_kernels.hip")
    body = k[k.index("static int launch_slots"):k.index("static int launch_nw")]
    low = sorted(int(s) for s in re.findall(r"launch_one<PREC, METHOD, (\d), NW, 5, 3>", body))
    gen = sorted(int(s) for s in re.findall(r"launch_one<PREC, METHOD, (\d), NW>", body))
    assert low == [1, 2, 3, 4] and gen == list(range(1, sc.K_SLOTS_MAX + 1))
    assert "code.dc_max <= 6 && code.dv_max <= 3" in body and "NW == 1 && METHOD <= 1" in body
    mw = k[k.index("static int launch_mw_slots"):k.index("static int launch_slots")]
    assert sorted(int(s) for s in re.findall(r"launch_mw<PREC, METHOD, (\d), NW>", mw)) == gen
    assert re.findall(r"launch_nw<(\d)>\(code", k) == ["1", "4"]
    capi = source("ldpc_capi_create.hip")
    assert "nw == 1 && dc_max <= 6 && dv_max <= 3 && slots <= 4" in capi
    assert "ctx->nw = N <= 64 ? 1 : 4;" in capi
    for name in ("ldpc_ring.hip", "ldpc_serve.hip"):
        t = source(name)
        assert "code.dc_max <= 6 && code.dv_max <= 3" in t, name
        assert "constexpr int D = kDcMax - 1, V = kDvMax;" in t, name
    g = source("ldpc_graph.hip")
    assert sorted(set(int(d) for d in re.findall(r"g_check<PREC, (\d+)><<<", g))) == [8, 16, 32]
    assert sorted(set(int(d) for d in re.findall(r"g_var<Real, (\d+)><<<", g))) == [4, 8, 16]
    assert sorted(set(int(d) for d in re.findall(r"g_var_bf<(\d+)><<<", g))) == [4, 8, 16]
    assert sc.graph_bodies(8, 4) == (8, 4) and sc.graph_bodies(9, 5) == (16, 8)
    assert sc.graph_bodies(16, 8) == (16, 8) and sc.graph_bodies(17, 9) == (32, 16)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_case_has_its_listed_shape(name):
    c = CASES[name]
    s = c.shape
    assert set(np.unique(c.H)) <= {0, 1}
    if c.expect is not None:
        E, dc, dv = c.expect
        assert (dc, dv) == (s["dc"], s["dv"]) and E in (None, s["E"]), (name, s)
    assert c.small == sc.fits_small(s["M"], s["N"], s["E"], s["dc"], s["dv"]), (name, s)
    M, N, rp, ci = c.csr
    assert rp[-1] == s["E"] == ci.size


def test_named_cases_keep_their_cells():
    """(slots, NW, generic, cols, rs, KB) of the cases other tests pick by name."""
    want = dict(d_8x32=(1, 1, True, False, 1, 3), a_16x64=(2, 1, True, False, 1, 6),
                e_24x64=(3, 1, True, False, 1, 5), l_31x63=(3, 1, True, False, 1, 4),
                b_48x64=(4, 1, True, True, 1, 2), c_32x64=(4, 1, True, True, 1, 4),
                j_13x65=(2, 4, True, False, 1, 7), i_24x96=(3, 4, True, False, 1, 9),
                m_56x80=(3, 4, True, False, 1, 3), k_37x101=(4, 4, True, False, 1, 8),
                h_160x224=(7, 4, True, False, 3, 8), g_250x256=(8, 4, True, False, 4, 1),
                f_64x128=(8, 4, True, False, 1, 8))
    for name, w in want.items():
        s = CASES[name].shape
        assert (s["slots"], s["NW"], s["generic"], s["cols"], s["rs"], s["KB"]) == w, (name, s)
    assert CASES["r_40x300"].shape["KB"] == 33
    z = CASES["z_empty"].H
    assert z.sum(0).min() == 0 and z.sum(1).min() == 0
    assert CASES["limit_40x120"].H.sum(1).min() == 1  # a degree-1 row
    for name in ("l_31x63", "k_37x101"):  # irregular: odd N, K % 8 != 0 or a degree-1 column
        H = CASES[name].H
        assert H.shape[1] % 2 == 1 and H.sum(0).min() == 1 and len(set(H.sum(0))) == 4


def test_table_reaches_every_small_code_cell(golden):
    reached = set()
    for name in SMALL:
        s = CASES[name].shape
        reached.add((s["NW"], s["generic"], s["cols"], s["slots"]))
    generic = {c for c in sc.small_cells() if c[1]}
    assert generic <= reached, sorted(generic - reached)
    # the low cells belong to the reference's own matrices (tests/golden)
    ref = golden("reference_data.npz")
    low = set()
    for n in ("decoder_h", "qa_h", "hData1", "hData2", "hData3", "hData4", "hData5"):
        H = ref[n]
        M, N = H.shape
        S, NW, dcn, dvn, cols = sc.kernel_shape(M, N, int(H.sum()), int(H.sum(1).max()),
                                                int(H.sum(0).max()))
        if (dcn, dvn) == (5, 3):
            low.add((NW, False, cols, S))
    assert reached | low >= sc.small_cells(), sorted(sc.small_cells() - reached - low)


def test_table_reaches_every_row_slot_count():
    assert {CASES[n].shape["rs"] for n in SMALL} == {1, 2, 3, 4}


def test_table_reaches_every_large_code_body_pair():
    reached = {CASES[n].shape["bodies"] for n in LARGE}
    reached |= {CASES[n].shape["bodies"] for n in SMALL}  # forced onto the large-code kernels
    want = {(dc, dv) for dc in (8, 16, 32) for dv in (4, 8, 16)}
    assert reached >= want, sorted(want - reached)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_oracle_sees_early_and_capped_frames(name):
    """Methods 0-2 at the cap of 20.  The small cases are counted with the
    oracle's sparse restatement (the GPU tests hold the kernels to the dense
    one); for the large cases both run and agree on every output
    (Case._oracle)."""
    c = CASES[name]
    counts = c.counts(sparse=c.small)
    for m, (early, capped) in counts.items():
        assert early > 0 and capped > 0, (name, m, counts)
