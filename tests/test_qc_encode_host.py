"""The quasi-cyclic encoder without a GPU: ldpc_plan_qc_encoder recognises the
two parity forms (a dual-diagonal core, a block lower triangular extension)
and refuses anything else by block row and column; ldpc_encode_qc, the host
executor of the step program the device encoder runs, yields codewords with a
zero syndrome and the data part untouched -- which, the parity part being
invertible, is the right codeword -- and agrees with codes.qc_encode where
that encoder applies."""
import re

import numpy as np
import pytest

import qc_encode_cases as qe
from ldpc_ece535a import _capi, codes


@pytest.mark.parametrize("name", qe.HOST_CASES + ("T24k",))
def test_plan_accepts(name):
    base, Z, core = qe.base_of(name)
    p = _capi.plan_qc_encoder(base, Z)
    assert p["encodable"], p
    assert p["core"] == core
    mb, nb = base.shape
    assert p["lds_bytes"] == -(-(nb + core) * Z // 16) * 16
    assert 1 <= p["levels"] <= mb + 2


def test_plan_levels():
    """A core takes three levels whatever its size; an extension row comes one
    level after the last parity block it reads; a triangular dual diagonal is
    one level per block row."""
    assert _capi.plan_qc_encoder(*qe.base_of("W27")[:2])["levels"] == 3
    assert _capi.plan_qc_encoder(*qe.base_of("W3")[:2])["levels"] == 3
    assert _capi.plan_qc_encoder(*qe.base_of("B")[:2])["levels"] == 12
    base = codes.qc_parity_core(4, 3, 12, 8, 3, 1)
    base[4:, :7] = -1
    for r in range(4, 7):            # extension rows that read the core alone: one level
        base[r, r] = 1
        base[r, r - 4] = 2
    assert _capi.plan_qc_encoder(base, 8)["levels"] == 4


@pytest.mark.parametrize("name", sorted(qe.refusals()))
def test_plan_refuses(name):
    base, Z, r, c = qe.refusals()[name]
    p = _capi.plan_qc_encoder(base, Z)
    assert not p["encodable"]
    assert re.search(r"block row %d, block column %d\b" % (r, c), p["reason"]), p["reason"]
    with pytest.raises(_capi.LdpcError, match="LDPC_EUNSUPPORTED.*block row %d, block column %d" % (r, c)):
        _capi.encode_qc(base, Z, np.zeros((1, (base.shape[1] - base.shape[0]) * Z), np.uint8))


def test_plan_refuses_short_core():
    """One entry above the diagonal makes no core (mc >= 3)."""
    base, Z = qe.base_of("A")[:2]
    base = base.copy()
    base[0, 1] = 0
    p = _capi.plan_qc_encoder(base, Z)
    assert not p["encodable"] and "block row 0, block column 1" in p["reason"]


def test_bad_description():
    base, Z, _ = qe.base_of("W7")
    base[2, 5] = Z
    with pytest.raises(_capi.LdpcError, match="LDPC_EINVAL"):
        _capi.plan_qc_encoder(base, Z)
    with pytest.raises(_capi.LdpcError, match="LDPC_EINVAL"):
        _capi.encode_qc(base, Z, np.zeros((1, 6 * Z), np.uint8))


@pytest.mark.parametrize("name", qe.HOST_CASES)
def test_encode_qc(name):
    base, Z, core = qe.base_of(name)
    mb = base.shape[0]
    data = qe.data_of(name, 5)
    cw = _capi.encode_qc(base, Z, data)
    assert cw.max() <= 1
    assert (cw[:, mb * Z:] == data).all()
    csr = codes.qc_expand(base, Z)
    assert (codes.syndrome_weight(csr, cw) == 0).all()
    if core == 0 and (np.diagonal(base[:, :mb]) == 0).all():
        assert (cw == codes.qc_encode(csr, data)).all()
    # bit 0 alone counts
    rng = np.random.Generator(np.random.PCG64(5))
    dirty = data | (rng.integers(0, 128, data.shape, np.uint8) << 1)
    assert (_capi.encode_qc(base, Z, dirty) == cw).all()


def test_encode_qc_is_linear_and_nontrivial():
    """The zero word encodes to zero, and a parity block is not constant."""
    base, Z, _ = qe.base_of("W27")
    K = 12 * Z
    assert not _capi.encode_qc(base, Z, np.zeros((1, K), np.uint8)).any()
    cw = _capi.encode_qc(base, Z, qe.data_of("W27", 5))
    assert cw[:, :12 * Z].any(axis=0).sum() > 6 * Z


def test_generator():
    """qc_parity_core: seeded, the shape asked for, and refused arguments."""
    a = codes.qc_parity_core(4, 6, 18, 16, 3, 25)
    assert (a == codes.qc_parity_core(4, 6, 18, 16, 3, 25)).all()
    assert (a != codes.qc_parity_core(4, 6, 18, 16, 3, 26)).any()
    assert a.shape == (10, 18) and a.min() >= -1 and a.max() < 16
    assert ((a[:, 10:] >= 0).sum(axis=0) == 3).all()
    assert (a[0, 0], a[3, 0], a[2, 0]) == (1, 1, 0) and (a[:4, 0] >= 0).sum() == 3
    for r in range(4, 10):
        assert a[r, r] >= 0 and (a[r, r + 1:10] < 0).all() and (a[r, :r] >= 0).sum() <= 2
    for bad in ((2, 0, 6, 8), (4, 0, 4, 8), (1, 2, 9, 8)):
        with pytest.raises(ValueError):
            codes.qc_parity_core(*bad, 3, 1)
    with pytest.raises(ValueError):
        codes.qc_parity_core(4, 0, 8, 8, 3, 1, x=3)
