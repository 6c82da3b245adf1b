"""GPU: the quasi-cyclic device encoder (ldpc_encode_device on a context made
by ldpc_create_qc, ldpc_aux.hip k_encode_qc) against the host executor of the
same step program (_capi.encode_qc), codes.qc_encode where it applies, and the
code itself (zero syndrome, data part intact: the codeword is unique), then the
chain it exists for: encode -> channel -> layered decode -> count, and the BER
sweep of a quasi-cyclic code.  The codes are synthetic (tests/qc_encode_cases.py)."""
import math

import numpy as np
import pytest

import qc_encode_cases as qe

pytestmark = pytest.mark.gpu

CANARY = 64


def _encode(dec, data, stream=None, calls=1):
    """Device codewords of `data` (B, K) bytes, written between two canaries."""
    import torch
    B = data.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(data)).cuda(0)
    buf = torch.full((CANARY + B * dec.N + CANARY,), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(calls):
        dec.encode_device(x.data_ptr(), B, buf.data_ptr() + CANARY,
                          None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    dec.synchronize()
    out = buf.cpu().numpy()
    assert (out[:CANARY] == 0xAA).all() and (out[-CANARY:] == 0xAA).all(), "canary overwritten"
    return out[CANARY:-CANARY].reshape(B, dec.N)


def _check(name, B, stream=None, calls=1):
    import ldpc_ece535a as L
    from ldpc_ece535a import _capi, codes
    base, Z, core = qe.base_of(name)
    mb = base.shape[0]
    assert _capi.plan_qc_encoder(base, Z)["core"] == core       # fails here without the feature
    dec = L.Decoder(qc=(base, Z))
    data = qe.data_of(name, B)
    ref = _capi.encode_qc(base, Z, data)
    csr = codes.qc_expand(base, Z)
    assert (codes.syndrome_weight(csr, ref) == 0).all()
    got = _encode(dec, data, stream, calls)
    np.testing.assert_array_equal(got, ref)
    assert (got[:, mb * Z:] == data).all()
    if core == 0:
        np.testing.assert_array_equal(got, codes.qc_encode(csr, data))
    # bit 0 alone counts: 0xFE is a zero, 0x03 a one
    dirty = np.where(data == 1, 0x03, 0xFE).astype(np.uint8)
    np.testing.assert_array_equal(_encode(dec, dirty), ref)
    dec.close()


@pytest.mark.parametrize("name", qe.GPU_CORE)
def test_core_cases(name):
    """W27: Z below a wave.  W96: 1.5 waves, shift Z - 1.  W7: b != 0, odd Z.
    W3: the smallest core.  X16: core and extension.  X384: six waves, a level
    wider than the block.  X16 also runs on a stream of the caller's."""
    import torch
    stream = torch.cuda.Stream(torch.device("cuda", 0)) if name == "X16" else None
    _check(name, qe.CORE[name][3], stream=stream)


@pytest.mark.parametrize("name", qe.TRIANGULAR)
def test_triangular_cases(name):
    """The lower-triangular dual diagonal (core 0): Z = 1 (E), Z = 1024 (F), a
    block row of degree 32 (G); A is encoded twice on one context, the second
    call reusing the uploaded program."""
    _check(name, 9, calls=2 if name == "A" else 1)


def test_frame_of_24k():
    """N = 24 576 bytes of LDS, 1024 threads."""
    _check("T24k", 2)


def test_frame_beyond_64k():
    """N = 69 632: more dynamic LDS than a kernel gets without asking."""
    _check("T68k", 2)


def test_frame_beyond_the_lds_is_refused():
    """N = 172 032 bytes do not fit a workgroup's LDS: refused with the size,
    and no fallback."""
    import torch
    import ldpc_ece535a as L
    from ldpc_ece535a import _capi
    base, Z, _ = qe.base_of("T168k")
    assert _capi.plan_qc_encoder(base, Z) == dict(encodable=True, core=0, levels=8, lds_bytes=172032)
    dec = L.Decoder(qc=(base, Z))
    x = torch.zeros((1, dec.K), dtype=torch.uint8, device="cuda:0")
    y = torch.zeros((1, dec.N), dtype=torch.uint8, device="cuda:0")
    for _ in range(2):      # the refusal is remembered
        with pytest.raises(L.LdpcError, match="LDPC_EUNSUPPORTED.*172032 bytes of LDS"):
            dec.encode_device(x.data_ptr(), 1, y.data_ptr())
    dec.close()


def test_rows_without_information():
    """A core row and an extension row with lam = 0."""
    _check("L0", 3)


def test_empty_batch_and_other_contexts():
    """B = 0 is a no-op; a quasi-cyclic context that is not encodable keeps
    today's answer."""
    import torch
    import ldpc_ece535a as L
    base, Z, _ = qe.base_of("W27")
    dec = L.Decoder(qc=(base, Z))
    dec.encode_device(None, 0, None)
    bad = base.copy()
    bad[11, 0] = 2
    d2 = L.Decoder(qc=(bad, Z))
    x = torch.zeros((1, d2.K), dtype=torch.uint8, device="cuda:0")
    y = torch.zeros((1, d2.N), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(L.LdpcError, match="staircase"):
        d2.encode_device(x.data_ptr(), 1, y.data_ptr())
    dec.close()
    d2.close()


def test_round_trip_on_the_device():
    """W27, 256 frames at 6 dB: random_bits -> encode_device -> bpsk_awgn ->
    decode_layered_device (scale 0.8125, f32, cap 10) -> count_bit_errors, all
    on one stream.  0 bit errors and 0 non-zero syndromes: the numpy
    restatement (tests/layered_ref.py, block-row plan) left no frame of this
    shape undecoded at 4, 6 and 8 dB, so 6 dB stands a 2 dB step clear."""
    import torch
    import ldpc_ece535a as L
    from ldpc_ece535a import _capi, ber, codes
    base, Z, _ = qe.base_of("W27")
    dec = L.Decoder(qc=(base, Z))
    B, N, K = 256, dec.N, dec.K
    dev = torch.device("cuda", 0)
    d_data = torch.empty((B, K), dtype=torch.uint8, device=dev)
    d_cw = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_tx = torch.empty((B, N), dtype=torch.float32, device=dev)
    d_bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_packed = torch.empty((B, dec.KB), dtype=torch.uint8, device=dev)
    d_synd = torch.empty(B, dtype=torch.int32, device=dev)
    d_err = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    _capi.random_bits(d_data.data_ptr(), B * K, 77, sp)
    dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr(), sp)
    _capi.bpsk_awgn(d_cw.data_ptr(), B * N, ber.sigma_of(6.0), 78, d_tx.data_ptr(), sp)
    dec.decode_layered_device(d_tx.data_ptr(), B, d_packed.data_ptr(), scale=0.8125, max_iters=10,
                              precision=L.PREC_F32, d_bits=d_bits.data_ptr(),
                              d_synd=d_synd.data_ptr(), stream=sp)
    _capi.count_bit_errors(d_bits.data_ptr(), d_cw.data_ptr(), N, B, d_err.data_ptr(), sp)
    stream.synchronize()
    cw = d_cw.cpu().numpy()
    data = d_data.cpu().numpy()
    assert 0.4 < data.mean() < 0.6
    assert (cw[:, 12 * Z:] == data).all()
    assert (codes.syndrome_weight(codes.qc_expand(base, Z), cw) == 0).all()
    err, synd = d_err.cpu().numpy(), d_synd.cpu().numpy()
    print("bit errors %d, frames with a non-zero syndrome %d" % (err.sum(), (synd > 0).sum()))
    assert err.sum() == 0 and (synd == 0).all()
    assert (np.packbits(data, axis=1) == d_packed.cpu().numpy()).all()
    dec.close()


def test_ber_sweep_of_a_qc_code():
    """ber.sweep on the --qc code of W27, grid [2, 6] dB, 256 frames, with the
    layered curve: every curve non-increasing, the layered one 0 at 6 dB, and
    the hard-decision curve within four binomial standard deviations of
    Q(1 / sigma)."""
    import ldpc_ece535a as L
    from ldpc_ece535a import ber
    (mc, me, nb, Z), _, seed, _ = qe.CORE["W27"]
    base, Z, label = ber.qc_code("%d,%d,%d,%d,%d,%d" % (mc, me, nb, Z, qe.INFO_DEG, seed))
    assert (base == qe.base_of("W27")[0]).all() and label.startswith("QC ")
    assert label.endswith("(synthetic base matrix)")
    dec = L.Decoder(qc=(base, Z))
    grid, frames = [2.0, 6.0], 256
    res = ber.sweep(dec, grid, frames, 10, seed=3, precision=L.PREC_F32, layered_scale=0.8125)
    assert set(res) == {"BPSK", "BitFlip", "LogDomainSimple", "SumProduct", ber.LAYERED}
    for name, r in res.items():
        print(name, r)
        assert r["ber"][1] <= r["ber"][0] and r["fer"][1] <= r["fer"][0], name
    assert res[ber.LAYERED]["ber"][1] == 0.0 and res[ber.LAYERED]["fer"][1] == 0
    n = frames * dec.N
    for db, got in zip(grid, res["BPSK"]["ber"]):
        p = 0.5 * math.erfc(1.0 / ber.sigma_of(db) / math.sqrt(2.0))
        print("BPSK %.1f dB: %.5f, Q(1/sigma) = %.5f, sd %.5f" % (db, got, p, math.sqrt(p * (1 - p) / n)))
        assert abs(got - p) <= 4.0 * math.sqrt(p * (1 - p) / n)
    dec.close()
