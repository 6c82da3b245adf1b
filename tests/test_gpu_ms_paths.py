"""Large-code min-sum runs on the narrow-chunk frame pipeline with
compressed check messages (ldpc_graph_msn.hip).  It must reproduce the
oracle exactly: the reference's fixtures on its own H forced onto the
large-code path (hard decisions, packed bytes, iterations, syndromes,
posteriors), the DVB-S2-like code against the sparse restatement, non-finite
samples, et_period 5, batches far larger than the pipeline's slots (every
slot recycled many times), and each knob and code shape that picks another
of its paths."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _decoder(env=None, **kw):
    import ldpc_ece535a as L
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return L.Decoder(**kw)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def gdec():
    return _decoder(force_graph=True)


@pytest.mark.parametrize("db", [0, 2, 4])
@pytest.mark.parametrize("iters", [5, 50])
def test_fixtures(gdec, golden, db, iters):
    fd = golden("frames_default.npz")
    out = gdec.decode(fd["db%d_llr" % db], method=0, max_iters=iters, want_llr=True)
    key = "db%d_m0_i%d" % (db, iters)
    for k in ("bits", "packed", "iters", "synd"):
        np.testing.assert_array_equal(out[k], fd[key + "_" + k], err_msg=k)
    np.testing.assert_array_equal(out["llr"], fd[key + "_post"])


@pytest.mark.parametrize("B", [1, 63, 65, 300, 5000])
def test_batches_and_et_period(gdec, B):
    from oracle import oracle as orc
    rng = np.random.default_rng(B)
    Hr = gdec.H
    x = 2.0 * __import__("ldpc_ece535a").encode(
        Hr, rng.integers(0, 2, size=(B, 32), dtype=np.uint8)) - 1.0
    db = rng.integers(0, 5, size=B)
    y = (x + np.sqrt(10.0 ** (-db / 10.0))[:, None] * rng.standard_normal(x.shape)).astype(
        np.float32)
    for et in (1, 5):
        out = gdec.decode(y, method=0, max_iters=50, et_period=et)
        ref = orc.decode_batch(0, Hr, y, 50, nthreads=16, et_period=et)
        for k in ("bits", "packed", "iters", "synd"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg="%s et=%d" % (k, et))


@pytest.mark.parametrize("method,precision", [(0, 0), (0, 1), (1, 0)],
                         ids=["minsum-f64", "minsum-f32", "sumproduct-f64"])
def test_work_limit_lowers_chunks_and_groups(gdec, method, precision):
    """ldpc_set_work_limit(1): no workspace fits, so the pipeline lowers its
    chunk count to the one chunk it always keeps (two frames in flight, every
    slot recycled 32 times over 65 frames) and the other path decodes in
    groups of 64 frames (64 + 1).  Every output equals the oracle's -- for f32
    its float restatement's."""
    from oracle import oracle as orc
    B = 65
    rng = np.random.default_rng(B)
    Hr = gdec.H
    x = 2.0 * __import__("ldpc_ece535a").encode(
        Hr, rng.integers(0, 2, size=(B, 32), dtype=np.uint8)) - 1.0
    db = rng.integers(0, 5, size=B)
    y = (x + np.sqrt(10.0 ** (-db / 10.0))[:, None] * rng.standard_normal(x.shape)).astype(
        np.float32)
    kw = {"real": "f32"} if precision == 1 else {}
    ref = orc.decode_batch(method, Hr, y, 50, nthreads=16, et_period=1, **kw)
    gdec.set_work_limit(1)
    try:
        out = gdec.decode(y, method=method, max_iters=50, et_period=1, precision=precision)
    finally:
        gdec.set_work_limit(0)
    for k in ("bits", "packed", "iters", "synd"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def test_non_finite(gdec):
    from oracle import oracle as orc
    rng = np.random.default_rng(3)
    y = rng.standard_normal((200, 64)).astype(np.float32)
    y[::7, 3] = np.inf
    y[1::5, 10] = -np.inf
    y[2::9, 20] = np.nan
    y[3::4, 30:34] = 0.0
    out = gdec.decode(y, method=0, max_iters=20, want_llr=True)
    ref = orc.decode_batch(0, gdec.H, y, 20, want_post=True)
    for k in ("bits", "iters", "synd"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(out["llr"], ref["post"])


def test_dvbs2_like_vs_sparse_oracle():
    from ldpc_ece535a import codes
    from oracle import oracle as orc
    csr = codes.dvbs2_like(0)
    d = _decoder(csr=csr)
    M, N, rp, ci = csr
    rng = np.random.Generator(np.random.PCG64(77))
    info = rng.integers(0, 2, size=(160, N - M), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    y = (x + np.sqrt(10 ** (-1.0 / 10)) * rng.standard_normal(x.shape)).astype(np.float32)
    out = d.decode(y, method=0, max_iters=50)
    ref = orc.decode_batch_sparse(0, rp, ci, M, N, y, 50, nthreads=16)
    for k in ("bits", "packed", "iters", "synd"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def _dvb_noisy(csr, B, seed, db):
    from ldpc_ece535a import codes
    M, N = csr[0], csr[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, N - M), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


@pytest.mark.parametrize("env", [{"LDPC_MSN_ORDER": "0"}, {"LDPC_MSN_ORDER": "1"},
                                 {"LDPC_MSN_CHUNKS": "5"}, {"LDPC_MSN_CHUNKS": "8"}],
                         ids=["identity-order", "residue-order", "5-chunks", "8-chunks"])
def test_narrow_variants_dvbs2(env):
    """The pipeline's knobs on the DVB-S2-like code: the identity storage
    order instead of the residue-class order (and the residue order forced),
    a chunk count that is not a multiple of 8 (no XCD placement) and a single
    chunk per XCD.  Packed bytes, bits, iterations and syndromes equal the
    sparse oracle's; posteriors equal the default settings' bit for bit (the
    posteriors themselves are pinned by test_fixtures)."""
    from ldpc_ece535a import codes
    from oracle import oracle as orc
    csr = codes.dvbs2_like(0)
    M, N, rp, ci = csr
    y = _dvb_noisy(csr, 96, 91, 1.5)
    out = _decoder(env, csr=csr).decode(y, method=0, max_iters=30, want_llr=True)
    ref = orc.decode_batch_sparse(0, rp, ci, M, N, y, 30, nthreads=16)
    for k in ("bits", "packed", "iters", "synd"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    base = _decoder(csr=csr).decode(y, method=0, max_iters=30, want_llr=True)
    np.testing.assert_array_equal(out["llr"].view(np.uint32), base["llr"].view(np.uint32))


def test_post_kernels_info_first_order():
    """The DVB-S2-like code with its columns in the ETSI order (information
    first): the staircase columns move in the residue-class storage order,
    so the outputs come from the separate msn_post / msn_cols kernels
    instead of the variable pass.  Equal to the sparse oracle; posteriors
    equal the same frames through the parity-first code (the same graph, its
    columns renamed)."""
    import ldpc_ece535a as L
    from ldpc_ece535a import codes
    from oracle import oracle as orc
    csr = codes.dvbs2_like(0)
    M, N, rp, ci = csr
    K = N - M
    newcol = np.where(ci >= M, ci - M, ci + K).astype(np.int64)  # parity -> K.., info -> 0..
    rows = np.repeat(np.arange(M), np.diff(rp))
    order = np.lexsort((newcol, rows))
    ci2 = newcol[order].astype(np.int32)
    csr2 = (M, N, rp, ci2)
    r = L._capi.plan_storage_order(csr2)
    assert r["order"] == 1 and not np.array_equal(r["cpos"][M:], np.arange(M, N))
    y = _dvb_noisy(csr, 96, 17, 1.5)
    y2 = np.concatenate([y[:, M:], y[:, :M]], axis=1)  # the same frames, columns renamed
    out = _decoder(csr=csr2).decode(y2, method=0, max_iters=30, want_llr=True)
    ref = orc.decode_batch_sparse(0, rp, ci2, M, N, y2, 30, nthreads=16)
    for k in ("bits", "packed", "iters", "synd"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    base = _decoder(csr=csr).decode(y, method=0, max_iters=30, want_llr=True)
    llr1 = np.concatenate([base["llr"][:, M:], base["llr"][:, :M]], axis=1)
    np.testing.assert_array_equal(out["llr"].view(np.uint32), llr1.view(np.uint32))


@pytest.mark.parametrize("hi_groups,hi_deg,dc", [(3, 8, 14), (5, 12, 20)],
                         ids=["dc14", "dc20"])
def test_high_check_degree_vs_sparse_oracle(hi_groups, hi_deg, dc):
    """Rate-3/4 IRA codes in the DVB-S2 style (N = 7200, 360-column groups)
    whose rows have 13-14 and 19-20 edges: the narrow pipeline's check pass
    then runs its 16- and 32-slot bodies with the slots past each block's
    degree masked, and its variable pass the degree-12 columns; every f64
    output equals the sparse oracle's and every f32 output (posteriors as bit
    patterns included) its float restatement's, at an Eb/N0 beyond the code's
    reach and at one within it."""
    from ldpc_ece535a import codes
    from oracle import oracle as orc
    table = codes.dvbs2_like_table(3, K=5400, N=7200, hi_groups=hi_groups, hi_deg=hi_deg,
                                   lo_deg=3)
    csr = codes.ira_from_table(table, 5400, 7200)
    M, N, rp, ci = csr
    assert int(np.diff(rp).max()) == dc
    d = _decoder(csr=csr)
    rng = np.random.Generator(np.random.PCG64(hi_deg))
    info = rng.integers(0, 2, size=(200, N - M), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
    n = rng.standard_normal(x.shape)
    for db in (3.0, 6.0):  # beyond / within the rate-3/4 code's reach
        y = (x + np.sqrt(10 ** (-db / 10)) * n).astype(np.float32)
        out = d.decode(y, method=0, max_iters=40, precision=0)
        ref = orc.decode_batch_sparse(0, rp, ci, M, N, y, 40, nthreads=16)
        for k in ("bits", "packed", "iters", "synd"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg="%s %g dB" % (k, db))
        # f32: the same arithmetic in float, all frames
        out = d.decode(y, method=0, max_iters=40, precision=1, want_llr=True)
        ref32 = orc.decode_batch_sparse(0, rp, ci, M, N, y, 40, nthreads=16, real="f32",
                                        want_post=True)
        for k in ("bits", "packed", "iters", "synd"):
            np.testing.assert_array_equal(out[k], ref32[k], err_msg="f32 %s %g dB" % (k, db))
        np.testing.assert_array_equal(out["llr"].view(np.uint32), ref32["post"].view(np.uint32))
    # 6 dB: most frames decode, in either arithmetic
    assert (ref["synd"] == 0).mean() > 0.5
    assert ((out["packed"] == np.packbits(info, axis=1)).all(axis=1)).mean() > 0.5
