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
    variable bodies 4 / 8 / 16.  The small-code rule and dispatch have one
    source each (kernel_shape in ldpc_kernels.hpp, dispatch_small in
    ldpc_dispatch.hpp), and no launcher states either again."""
    # the one shape rule, condition by condition
    hpp = source("ldpc_kernels.hpp")
    assert "const bool low = nw == 1 && dc_max <= 6 && dv_max <= 3 && slots <= 4;" in hpp
    assert "const int dcn = low ? 5 : kDcMax - 1, dvn = low ? 3 : kDvMax;" in hpp
    assert "return KernelShape{low, dcn, dvn, cols_form(1, slots, nw, dvn)};" in hpp
    assert "return method == 1 && nw == 1 && dvn <= slots;" in hpp
    frame = source("ldpc_frame.hpp")
    assert "return cols_form(METHOD, S, NW, DVN);" in frame
    # ... is stated nowhere else, and the restatement agrees: low cells at 1..4 slots of NW = 1
    for name in sorted(os.listdir(CSRC)):
        if os.path.isfile(os.path.join(CSRC, name)) and name != "ldpc_kernels.hpp":
            t = source(name)
            assert "dc_max <= 6" not in t and "dv_max <= 3" not in t, name
            assert "DVN <= S" not in t and "dvn <= slots" not in t, name
    gen = list(range(1, sc.K_SLOTS_MAX + 1))
    assert [s for s in gen if sc.kernel_shape(1, 64, 64 * s, 6, 3)[2:4] == (5, 3)] == [1, 2, 3, 4]
    assert not [s for s in gen if sc.kernel_shape(1, 65, 64 * s, 6, 3)[2:4] == (5, 3)]
    assert all(sc.kernel_shape(1, 64, 64 * s, dc, dv)[2:4] == (7, 4)
               for s in gen for dc, dv in ((7, 3), (6, 4)))
    # the one dispatcher: slots 1..8, a cell instantiated only below the caller's largest
    # slot count and, for the low loops, only where the rule has a low cell; NW 1 and 4
    d = source("ldpc_dispatch.hpp")
    by = d[d.index("int by_slots("):d.index("int by_shape(")]
    cases = re.findall(r"case (\d): return at\(std::integral_constant<int, (\d)>\{\}\);", by)
    assert [(int(a), int(b)) for a, b in cases] == [(s, s) for s in gen]
    assert "if constexpr (S <= MAXS && cell_shape(NW, S, LOW).low == LOW)" in by
    assert "return f(SmallCell<PREC, METHOD, S, NW, LOW>{});" in by
    assert "return kernel_shape(nw, slots, low ? 0 : kDcMax, low ? 0 : kDvMax);" in d
    assert ("static constexpr int DCN = cell_shape(NW, S, LOW).dcn, DVN = cell_shape(NW, S, LOW).dvn;"
            in d)
    assert re.findall(r"if \(nw == (\d)\) return dispatch::by_method<MAXS, (\d)>\(", d) == [
        ("1", "1"), ("4", "4")]
    # the launchers: each goes through the dispatcher with the code's shape, up to its own
    # largest slot count (the server's is 4); the multi-wave kernel has 1..8, generic only
    own = "kernel_shape(nw, slots, code.dc_max, code.dv_max)"
    k = source("ldpc_kernels.hip")
    assert "constexpr int kBatchSlotsMax = kSlotsMax;" in k
    calls = re.findall(r"dispatch_small<kBatchSlotsMax>\(method, prec, slots, nw,\s*([^;]*?),\s*"
                       r"(Launch\w+)\{code, a, st\}\);", k)
    assert calls == [("kernel_shape(nw, slots, kDcMax, kDvMax)", "LaunchMw"), (own, "LaunchOne")]
    assert "return launch_mw<C::PREC, C::METHOD, C::S, C::NW>(code, a, st);" in k
    assert k.count("launch_one<C::PREC, C::METHOD, C::S, C::NW, C::DCN, C::DVN, ") == 2
    ring = source("ldpc_ring.hip")
    assert "constexpr int kRingSlotsMax = kSlotsMax;" in ring
    assert re.search(r"dispatch_small<kRingSlotsMax>\(\s*method, prec, slots, nw, %s," % re.escape(own),
                     ring)
    assert "launch_r<C::PREC, C::METHOD, C::S, C::NW, C::DCN, C::DVN, ring_minb<C>()>(" in ring
    serve = source("ldpc_serve.hip")
    assert constant(serve, "kServeSlotsMax") == 4
    assert re.search(r"dispatch_small<kServeSlotsMax>\(\s*method, prec, slots, nw, %s," % re.escape(own),
                     serve)
    assert "launch_s<C::PREC, C::METHOD, C::S, C::NW, C::DCN, C::DVN>(" in serve
    capi = source("ldpc_capi_create.hip")
    assert "ldpc::kernel_shape(nw, slots, code.dc_max, code.dv_max);" in capi
    assert "slots, nw, shape.dcn, shape.dvn,\n" in capi and "shape.cols, search);" in capi
    assert "ctx->nw = N <= 64 ? 1 : 4;" in capi
    assert sum(source(n).count("#define LDPC_TP_MINB") for n in os.listdir(CSRC)
               if os.path.isfile(os.path.join(CSRC, n))) == 1
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
