"""Host: tests/gf2_ref.py against the host encoder (makeParityCheck) on the
N = 2M golden matrices, and the codes of tests/encode_cases.py: full rank,
column weight 3, degrees a context accepts, shapes that cover what their
comments say."""
import numpy as np
import pytest

import encode_cases as ec
import gf2_ref

import ldpc_ece535a as L
from ldpc_ece535a import codes


def test_eliminate_and_rank():
    A = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]], np.uint8)      # row 2 = row 0 + row 1
    assert gf2_ref.rank(A) == 2 and gf2_ref.rank(np.eye(5, dtype=np.uint8)) == 5
    R, piv = gf2_ref.eliminate(A, 3)
    assert piv == [0, 1] and not R[2].any()
    with pytest.raises(ValueError, match="dependent"):
        gf2_ref.encode(np.concatenate([A, np.eye(3, dtype=np.uint8)], axis=1), np.zeros((1, 3)))


@pytest.mark.parametrize("name", ["decoder_h", "qa_h", "hData1", "hData2", "hData3", "hData4",
                                  "hData5"])
def test_gf2_encode_equals_host_encoder(golden, name):
    H = golden("reference_data.npz")[name]
    Hr, _ = L.reorder_h(H)
    M, N = Hr.shape
    assert N == 2 * M
    data = ec.data_for(N - M, N - M + 3)
    cw = gf2_ref.encode(Hr, data)
    assert (cw == L.encode(Hr, data)).all()
    assert not gf2_ref.syndrome(Hr, cw).any() and (cw[:, M:] == data).all()
    assert gf2_ref.syndrome(Hr, cw ^ np.eye(N, dtype=np.uint8)[:1]).any()


@pytest.mark.parametrize("M,N,seed", ec.SMALL + [ec.REFUSED])
def test_small_codes(M, N, seed):
    H = ec.small_code(M, N, seed)
    assert H.shape == (M, N) and (H.sum(axis=0) == 3).all()
    assert gf2_ref.rank(H) == M
    assert H.sum(axis=1).max() <= 32          # the row-degree limit of a context
    assert (ec.small_code(M, N, seed) == H).all()
    Hr, _ = L.reorder_h(H)
    cw = gf2_ref.encode(Hr, ec.data_for(N - M, 3))
    assert not gf2_ref.syndrome(Hr, cw).any()


def test_small_shapes_cover_what_they_name():
    K = [N - M for M, N, _ in ec.SMALL]
    assert sorted({(k + 63) // 64 for k in K}) == [1, 2, 3, 4]
    assert {64, 65, 128, 129, 192, 225, 256} <= set(K) and max(K) == 256
    assert sorted({(M + 63) // 64 for M, _, _ in ec.SMALL}) == [1, 2, 4, 5]
    assert ec.REFUSED[1] - ec.REFUSED[0] == 257
    # beyond the small-code decoders, so the context takes the large-code path
    assert any(N > 256 and N - M <= 256 for M, N, _ in ec.SMALL)


def test_data_sets():
    for K in (50, 225, 256):
        d = ec.data_for(K, 333)
        assert not d[0].any() and d[1].all() and (d[2:K + 2] == np.eye(K, dtype=np.uint8)).all()
        assert set(np.unique(d[K + 2:])) == {0, 1}
    d = ec.data_for(64, 3)
    assert not d[0].any() and d[1].all() and 0 < d[2].sum() < 64
    assert ec.data_for(64, 1).shape == (1, 64)


@pytest.mark.parametrize("M,K,kind", ec.IRA)
def test_ira_codes(M, K, kind):
    csr = ec.ira_code(M, K, kind)
    _, N, rp, ci = csr
    assert N == M + K and N > 256                  # no dense H in the context: the IRA rule
    deg = np.diff(rp)
    assert deg.max() <= 32 and np.bincount(ci, minlength=N).max() <= 16
    info = np.array([(ci[rp[j]:rp[j + 1]] >= M).sum() for j in range(M)])
    for j in range(M):
        row = ci[rp[j]:rp[j + 1]]
        assert (np.diff(row) > 0).all()
        assert list(row[row < M]) == ([j - 1, j] if j else [0])
    if kind == "empty_rows":
        assert (info[1::3] == 0).all() and (info == 0).sum() >= M // 3
    if kind == "one_row":
        assert (info > 0).sum() == 1 and info[613] == 30
    cw = codes.ira_encode(csr, ec.data_for(K, 37))
    assert (codes.syndrome_weight(csr, cw) == 0).all()
    # the reference is the GF(2) solution here too
    H = np.zeros((M, N), np.uint8)
    H[np.repeat(np.arange(M), deg), ci] = 1
    assert (gf2_ref.encode(H, ec.data_for(K, 37)) == cw).all()


def test_ira_shapes_cover_what_they_name():
    Ms = [M for M, _, _ in ec.IRA]
    assert min(Ms) < 256 and 256 in Ms and any(M % 256 for M in Ms if M > 256)
    assert {(M + 255) // 256 for M in Ms} == {1, 2, 4}
