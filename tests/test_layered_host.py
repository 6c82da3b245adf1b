"""The layered decoder without a GPU: the layer planner (ldpc_plan_layers),
the numpy restatement of the contract (tests/layered_ref.py) pinned by a
scalar transcription, and the reason for the feature as a property of that
restatement against the oracle's flooding min-sum."""
import numpy as np
import pytest

import layered_ref as lref
import ldpc_ece535a as L
from ldpc_ece535a import codes
from shape_cases import degree_limit_code, dense_to_csr, same_bits

LDS_LIMIT = 163840


def _default_csr(golden):
    Hr = golden("frames_default.npz")["H_reordered"]
    rp, ci = dense_to_csr(Hr)
    return Hr.shape[0], Hr.shape[1], rp, ci


def _plan_codes(golden):
    return {"default": _default_csr(golden), "n720": lref.ira_code(360, 720, 1),
            "n2160": lref.ira_code(1080, 2160, 2), "limits": degree_limit_code()[0]}


@pytest.mark.parametrize("name", ["default", "n720", "n2160", "limits"])
@pytest.mark.parametrize("prec", [0, 1])
def test_plan_layers(golden, name, prec):
    csr = _plan_codes(golden)[name]
    M, N, rp, ci = csr
    p = L.plan_layers(csr, precision=prec)
    plan, nl = p["layer_of_row"], p["n_layers"]
    assert p["fits"] and plan.shape == (M,)
    assert plan.min() == 0 and plan.max() == nl - 1          # every row in one layer of [0, L)
    for layer in range(nl):
        cols = np.concatenate([ci[rp[j]:rp[j + 1]] for j in np.flatnonzero(plan == layer)])
        assert cols.size == np.unique(cols).size, "layer %d holds a column twice" % layer
    dv_max = np.bincount(ci, minlength=N).max()
    ff = int(lref.first_fit(csr).max()) + 1
    print("%s: L = %d, first fit %d, dv_max %d, %d bytes, %d threads" % (
        name, nl, ff, dv_max, p["lds_bytes"], p["threads"]))
    assert dv_max <= nl <= ff
    again = L.plan_layers(csr, precision=prec)
    assert (again["layer_of_row"] == plan).all() and again["n_layers"] == nl
    assert 0 < p["lds_bytes"] <= LDS_LIMIT
    assert p["threads"] % 64 == 0 and 64 <= p["threads"] <= 1024
    real = 4 if prec == 1 else 8
    assert p["lds_bytes"] >= real * (N + rp[M]) + N + 128     # LQ, R, decisions, reduction words


def test_first_fit_counts(golden):
    """What the planner must not exceed, for the four codes."""
    got = {k: int(lref.first_fit(c).max()) + 1 for k, c in _plan_codes(golden).items()}
    assert got == {"default": 7, "n720": 14, "n2160": 14, "limits": 16}


def test_plan_layers_does_not_fit():
    csr = codes.dvbs2_like(0)
    M, N, rp, ci = csr
    for prec, real in ((0, 8), (1, 4)):
        p = L.plan_layers(csr, precision=prec)
        assert not p["fits"]
        assert p["lds_bytes"] >= real * (N + rp[M]) + N + 128 > LDS_LIMIT
        assert p["n_layers"] >= np.bincount(ci, minlength=N).max()


def test_plan_layers_bad_arguments():
    rp = np.array([0, 2, 4], np.int32)
    good = (2, 4, rp, np.array([0, 1, 2, 3], np.int32))
    assert L.plan_layers(good)["n_layers"] == 1
    bad = [
        (2, 4, rp, np.array([1, 0, 2, 3], np.int32)),   # not ascending
        (2, 4, rp, np.array([0, 1, 2, 4], np.int32)),   # out of range
        (2, 4, np.array([0, 3, 2], np.int32), np.array([0, 1, 2, 3], np.int32)),
        (4, 4, np.array([0, 1, 2, 3, 4], np.int32), np.arange(4, dtype=np.int32)),  # M >= N
    ]
    for csr in bad:
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*CSR H must be"):
            L.plan_layers(csr)
    for prec in (-1, 4):
        with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*precision"):
            L.plan_layers(good, precision=prec)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.8125])
def test_restatement_equals_scalar_transcription(golden, prec, scale):
    fd = golden("frames_default.npz")
    csr = _default_csr(golden)
    plan = lref.first_fit(csr)
    y = np.concatenate([fd["db0_llr"][:3], fd["db2_llr"][:3], fd["db4_llr"][:2]]).copy()
    y[1, 3] = np.inf
    y[2, 10] = -np.inf
    y[4, 20] = np.nan
    y[5, 30:34] = 0.0
    y[6, 40:44] = -0.0
    for kw in (dict(max_iters=12), dict(max_iters=20, et_period=3, polarity=-1.0)):
        a = lref.decode(csr, plan, y, scale=scale, precision=prec, **kw)
        b = lref.decode_scalar(csr, plan, y, scale=scale, precision=prec, **kw)
        for k in lref.KEYS:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        same_bits(a["llr"], b["llr"], what=str(kw))
        if kw.get("polarity", 1.0) > 0:                  # inverted frames all reach the cap
            assert len(set(a["iters"])) > 1, a["iters"]  # frames of more than one length


def test_layered_beats_flooding_on_n720():
    """N = 720, seed 5, 128 frames, 2 dB, cap 50: the row-serial schedule
    leaves no more frames undecoded than the oracle's flooding min-sum and
    needs fewer iterations; the normalisation leaves fewer still."""
    from oracle import oracle as orc
    csr = lref.ira_code(360, 720, 1)
    M, N, rp, ci = csr
    y = lref.noisy(csr, 128, 2.0, 5)
    flood = orc.decode_batch_sparse(0, rp, ci, M, N, y, 50, nthreads=16)
    plan = L.plan_layers(csr)["layer_of_row"]
    lay1 = lref.decode(csr, plan, y, 50, scale=1.0)
    layn = lref.decode(csr, plan, y, 50, scale=0.8125)
    fails = [int((r["synd"] != 0).sum()) for r in (flood, lay1, layn)]
    means = [float(r["iters"].mean()) for r in (flood, lay1, layn)]
    print("frames with a non-zero syndrome (flooding, layered, layered 0.8125):", fails)
    print("mean iterations:", means)
    assert fails[1] <= fails[0]
    assert means[1] < means[0]
    assert fails[2] < fails[1]
