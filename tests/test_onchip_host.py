"""Host side of the on-chip decode path (LDPC_FLAG_ONCHIP, ldpc_plan_onchip):
which codes fit one workgroup's LDS, and how a context that was asked for the
path on a code that does not fit is refused -- decided from the code's shape,
before any device is looked up, so none of this needs a GPU."""
import numpy as np
import pytest

import ldpc_ece535a as L
from ldpc_ece535a import _capi, codes

LDS_LIMIT = 163840


def _shape(csr):
    M, N, rp, ci = csr
    return (M, N, int(rp[M]), int(np.diff(rp).max()), int(np.bincount(ci, minlength=N).max()))


@pytest.fixture(scope="module")
def n720():
    t = codes.dvbs2_like_table(3, K=360, N=720, hi_groups=1, hi_deg=6, lo_deg=3)
    return codes.ira_from_table(t, 360, 720)


@pytest.fixture(scope="module")
def n2160():
    t = codes.dvbs2_like_table(3, K=1080, N=2160, hi_groups=2, hi_deg=6, lo_deg=3)
    return codes.ira_from_table(t, 1080, 2160)


def test_codes_are_the_issue_ones(n720, n2160):
    assert _shape(n720) == (360, 720, 2879, 8, 6)
    assert _shape(n2160) == (1080, 2160, 7559, 7, 6)


@pytest.mark.parametrize("prec", [0, 1, 2, 3])
@pytest.mark.parametrize("method", [0, 1])
def test_plan_fits_mid_size_codes(n720, n2160, method, prec):
    for csr in (n720, n2160):
        r = _capi.plan_onchip(*_shape(csr), method=method, precision=prec)
        assert r["fits"], r
        real = 4 if prec == 1 else 8
        assert 2 * real * _shape(csr)[2] < r["lds_bytes"] <= LDS_LIMIT
        assert r["threads"] % 64 == 0 and 64 <= r["threads"] <= 1024


def test_plan_refuses_large_code_and_degrees(n720):
    big = _shape(codes.dvbs2_like(0))
    for method in (0, 1):
        for prec in range(4):
            r = _capi.plan_onchip(*big, method=method, precision=prec)
            assert not r["fits"] and r["lds_bytes"] > LDS_LIMIT
    M, N, E, dc, dv = _shape(n720)
    assert _capi.plan_onchip(M, N, E, 32, 16)["fits"]
    assert not _capi.plan_onchip(M, N, E, 33, dv)["fits"]
    assert not _capi.plan_onchip(M, N, E, dc, 17)["fits"]


def test_plan_bad_arguments(n720):
    M, N, E, dc, dv = _shape(n720)
    for kw in (dict(method=2), dict(method=3), dict(precision=4), dict(precision=-1)):
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL"):
            _capi.plan_onchip(M, N, E, dc, dv, **kw)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL"):
        _capi.plan_onchip(N, M, E, dc, dv)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL"):
        _capi.plan_onchip(M, N, 0, dc, dv)


def test_create_refuses_code_that_does_not_fit():
    """The refusal names the LDS bytes needed and the limit, and comes before
    the device lookup: the same message with or without a GPU."""
    csr = codes.dvbs2_like(0)
    needs = {_capi.plan_onchip(*_shape(csr), method=m, precision=p)["lds_bytes"]
             for m in (0, 1) for p in range(4)}
    with pytest.raises(L.LdpcError) as ei:
        L.Decoder(csr=csr, onchip=True)
    msg = str(ei.value)
    assert "LDS" in msg and str(LDS_LIMIT) in msg and any(str(n) in msg for n in needs), msg


def test_create_refuses_degrees():
    # one row of degree 33 (beyond the kernels' 32)
    M, N = 4, 40
    rows = [list(range(33)), [33, 34], [35, 36], [37, 38, 39]]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    with pytest.raises(L.LdpcError, match="degrees"):
        L.Decoder(csr=(M, N, rp, ci), onchip=True)


def test_onchip_and_force_graph_exclude_each_other(n720):
    with pytest.raises(L.LdpcError, match="exclude"):
        L.Decoder(onchip=True, force_graph=True)
    with pytest.raises(L.LdpcError, match="exclude"):
        L.Decoder(csr=n720, onchip=True, force_graph=True)
