"""Host side of the quasi-cyclic codes (ldpc_plan_qc, codes.qc_*): expansion,
threads, the LDS formula and the fit rule, refusals.  No GPU."""
import numpy as np
import pytest

import ldpc_ece535a as L
from ldpc_ece535a import codes

import qc_cases as qc

LDS_LIMIT = 163840


def a16(x):
    return (x + 15) // 16 * 16


def frame_bytes(N, E, prec):
    """The header's formula for lds_bytes."""
    real = 4 if prec == 1 else 8
    return a16(N * real) + a16(E * real) + a16(N) + 128


@pytest.mark.parametrize("name", ["A", "B", "E", "G"])
def test_expansion(name):
    base, Z = qc.base_of(name)
    H, (M, N, rp, ci) = qc.rolled(base, Z)
    if name != "G":
        assert (N, int(rp[M])) == qc.TABLE[name][1]
    for got in (L.plan_qc(base, Z)["csr"], codes.qc_expand(base, Z)):
        assert got[0] == M and got[1] == N
        np.testing.assert_array_equal(got[2], rp)
        np.testing.assert_array_equal(got[3], ci)
        assert got[2].dtype == np.int32 and got[3].dtype == np.int32
        for j in range(M):
            assert (np.diff(got[3][got[2][j]:got[2][j + 1]]) > 0).all(), j
    # row r * Z + i, base entry (r, c) = s: a one at column c * Z + (i + s) mod Z
    r, c = np.argwhere(base >= 0)[-1]
    i = Z - 1
    assert H[r * Z + i, c * Z + (i + base[r, c]) % Z] == 1


def test_case_g_degrees():
    base, Z = qc.base_of("G")
    H, _ = qc.rolled(base, Z)
    dc = H.sum(axis=1).reshape(4, Z)
    assert (dc == np.array([32, 12, 23, 1])[:, None]).all()
    assert H.sum(axis=0)[3 * Z:4 * Z].tolist() == [1] * Z
    assert {0, Z - 1} <= set(base[0, 4:].tolist())
    assert L.plan_qc(base, Z)["fits"]


@pytest.mark.parametrize("Z,threads", [(1, 64), (27, 64), (64, 64), (96, 128), (384, 384),
                                       (1024, 1024)])
def test_threads(Z, threads):
    base = codes.qc_dual_diagonal(2, 5, Z, 2, 9)
    assert L.plan_qc(base, Z)["threads"] == threads == 64 * -(-Z // 64)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F", "G"])
def test_lds_bytes_is_the_documented_formula(name, prec):
    base, Z = qc.base_of(name)
    p = L.plan_qc(base, Z, precision=prec)
    M, N, rp, ci = p["csr"]
    assert p["lds_bytes"] == frame_bytes(N, int(rp[M]), prec)
    assert p["fits"] == (p["lds_bytes"] <= LDS_LIMIT)
    assert p["fits"] or (name, prec) == ("F", 0)     # F is the float case


def test_fit_boundary():
    inside, beyond = qc.boundary_base(39), qc.boundary_base(40)
    p = L.plan_qc(inside, 384)
    assert p["fits"] and p["lds_bytes"] == 161408 == frame_bytes(4608, 39 * 384, 0) <= LDS_LIMIT
    p = L.plan_qc(beyond, 384)
    assert not p["fits"] and p["lds_bytes"] == 164480 == frame_bytes(4608, 40 * 384, 0) > LDS_LIMIT
    assert p["csr"][3].size == 40 * 384          # the expansion is written either way
    p = L.plan_qc(beyond, 384, precision=1)
    assert p["fits"] and p["lds_bytes"] == frame_bytes(4608, 40 * 384, 1)


def test_refusals():
    ok = np.array([[0, 1, -1], [-1, 2, 0]], np.int32)
    assert L.plan_qc(ok, 3)["csr"][3].size == 12
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*Z = 0"):
        L.plan_qc(np.array([[-1, -1]], np.int32), 0)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*Z = 1025"):
        L.plan_qc(ok, 1025)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*\(1, 1\).*shift 3 "):
        L.plan_qc(np.array([[0, 1, -1], [-1, 3, 0]], np.int32), 3)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*\(0, 2\).*shift -2 "):
        L.plan_qc(np.array([[0, 1, -2], [-1, 2, 0]], np.int32), 3)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*at least one row"):
        L.plan_qc(np.zeros((0, 3), np.int32), 3)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*precision"):
        L.plan_qc(ok, 3, precision=7)


def test_create_refusals_need_no_gpu():
    """What ldpc_create* refuse before they look for a device."""
    ok = np.array([[0, 1, -1], [-1, 2, 0]], np.int32)
    with pytest.raises(L.LdpcError, match=r"ldpc_create_qc failed.*shift 3 "):
        L.Decoder(qc=(np.array([[0, 3, -1], [-1, 2, 0]], np.int32), 3))
    with pytest.raises(L.LdpcError, match="a base matrix is two-dimensional"):
        L.Decoder(qc=(np.arange(3), 3))
    with pytest.raises(L.LdpcError, match="ldpc_create_csr failed.*LDPC_FLAG_QC_TABLES"):
        L.Decoder(csr=codes.qc_expand(ok, 3), qc_tables=True)
    with pytest.raises(L.LdpcError, match="ldpc_create failed.*LDPC_FLAG_QC_TABLES"):
        L.Decoder(qc_tables=True)


def test_a_base_row_of_degree_33_does_not_fit():
    base = np.full((2, 40), -1, np.int32)
    base[0, :33] = 0
    base[1, 30:] = 1
    p = L.plan_qc(base, 4)
    assert not p["fits"] and p["lds_bytes"] == frame_bytes(160, 43 * 4, 0)
    base[0, 32] = -1
    assert L.plan_qc(base, 4)["fits"]


def test_generator_and_encoder():
    S = codes.qc_dual_diagonal(6, 12, 64, 3, 1)
    assert S.shape == (6, 12) and S.dtype == np.int32
    assert ((S[:, 6:] >= 0).sum(axis=0) == 3).all() and (S >= -1).all() and (S < 64).all()
    par = np.full((6, 6), -1)
    par[np.arange(6), np.arange(6)] = 0
    par[np.arange(1, 6), np.arange(5)] = 0
    assert (S[:, :6] == par).all()
    assert (S == codes.qc_dual_diagonal(6, 12, 64, 3, 1)).all()
    assert (S != codes.qc_dual_diagonal(6, 12, 64, 3, 2)).any()
    csr = codes.qc_expand(S, 64)
    info = np.random.Generator(np.random.PCG64(3)).integers(0, 2, (5, 384), np.uint8)
    cw = codes.qc_encode(csr, info)
    assert (cw[:, 384:] == info).all() and not codes.syndrome_weight(csr, cw).any()
    with pytest.raises(ValueError):               # an upper-triangular parity part
        codes.qc_encode(codes.qc_expand(np.array([[0, 0, 1], [-1, 0, 2]]), 4),
                        np.zeros((1, 4), np.uint8))
