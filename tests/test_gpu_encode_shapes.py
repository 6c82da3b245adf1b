"""GPU: ldpc_encode_device over the shapes of tests/encode_cases.py -- every
instantiation of k_encode_small (one to four data words, full and partial),
one to five passes of its row loop, rates other than 1/2, and k_encode_ira
with idle threads, ragged segments and rows without information bits --
against the unique GF(2) solution (tests/gf2_ref.py, pinned on the CPU by
tests/test_encode_cases_host.py) and the host IRA encoder.

The data and codeword buffers carry 64 sentinel bytes behind them."""
import numpy as np
import pytest

import encode_cases as ec
import gf2_ref

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0xA5


def _encode(dec, data):
    """Device codewords of (B, K) data; the input may carry high bits."""
    import torch
    B = data.shape[0]
    x = torch.full((data.size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    x[:data.size] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).cuda(0)
    cw = torch.full((B * dec.N + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dec.encode_device(x.data_ptr(), B, cw.data_ptr())
    dec.synchronize()
    got = cw.cpu().numpy()
    assert (got[B * dec.N:] == SENTINEL).all(), "sentinel behind the codewords overwritten"
    assert (x.cpu().numpy()[:data.size] == data.reshape(-1)).all()
    return got[:B * dec.N].reshape(B, dec.N)


_small = {}


def _small_case(golden, key):
    """(decoder, {B: (data, reference codewords)}) of a small code, built once."""
    import ldpc_ece535a as L
    if key not in _small:
        H = golden("reference_data.npz")[ec.GOLDEN] if key == ec.GOLDEN else ec.small_code(*key)
        dec = L.Decoder(H)
        refs = {}
        for B in ec.BATCHES:
            data = ec.data_for(dec.K, B)
            refs[B] = (data, gf2_ref.encode(dec.H, data))
        _small[key] = (dec, refs)
    return _small[key]


@pytest.mark.parametrize("B", ec.BATCHES)
@pytest.mark.parametrize("key", [ec.GOLDEN] + ec.SMALL, ids=str)
def test_encode_small_equals_gf2_solution(golden, key, B):
    dec, refs = _small_case(golden, key)
    if key != ec.GOLDEN:
        assert (dec.M, dec.N) == key[:2]
    data, want = refs[B]
    got = _encode(dec, data)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d bytes differ; first: frame %d, column %d (M = %d)" % (
        len(bad), bad[0][0], bad[0][1], dec.M)
    if B == ec.BATCHES[-1]:
        # only bit 0 of a data byte is read, and the codeword holds 0 / 1
        hi = (np.arange(data.size, dtype=np.int64).reshape(data.shape) * 2 & 0xFE).astype(np.uint8)
        assert (_encode(dec, data | hi) == want).all()


def test_unit_vectors_read_the_matrix_back(golden):
    """The parity of unit vector i is column i of A = H_p^-1 H_d."""
    dec, refs = _small_case(golden, ec.SMALL[5])          # K = 225: four words, the last partial
    data, want = refs[333]
    K, M = dec.K, dec.M
    assert (data[2:K + 2] == np.eye(K, dtype=np.uint8)).all()
    A = want[2:K + 2, :M].T                                # (M, K)
    Hp, Hd = dec.H[:, :M].astype(np.int64), dec.H[:, M:].astype(np.int64)
    assert ((Hp @ A) & 1 == Hd).all()
    assert (_encode(dec, data)[2:K + 2, :M].T == A).all()


def test_k_257_falls_to_the_staircase_rule():
    """K = 257 is past the small rule (K <= 256 is a condition of the code, not
    a measurement): a dense code without the staircase has no device encoder."""
    import torch
    import ldpc_ece535a as L
    M, N, seed = ec.REFUSED
    dec = L.Decoder(ec.small_code(M, N, seed))
    assert dec.K == 257
    x = torch.zeros((1, dec.K), dtype=torch.uint8, device="cuda:0")
    y = torch.full((1, dec.N), SENTINEL, dtype=torch.uint8, device="cuda:0")
    for _ in range(2):                                     # the refusal is remembered
        with pytest.raises(L.LdpcError, match="large code without the accumulator staircase in "
                                              "columns 0..M-1: no device encoder"):
            dec.encode_device(x.data_ptr(), 1, y.data_ptr())
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("B", ec.IRA_BATCHES)
@pytest.mark.parametrize("M,K,kind", ec.IRA)
def test_encode_ira_equals_host_encoder(M, K, kind, B):
    import ldpc_ece535a as L
    from ldpc_ece535a import codes
    csr = ec.ira_code(M, K, kind)
    dec = L.Decoder(csr=csr)
    assert (dec.M, dec.K) == (M, K)
    data = ec.data_for(K, B)
    got = _encode(dec, data)
    want = codes.ira_encode(csr, data)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d bytes differ; first: frame %d, column %d (M = %d)" % (
        len(bad), bad[0][0], bad[0][1], M)
    assert (codes.syndrome_weight(csr, got) == 0).all()
