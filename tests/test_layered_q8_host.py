"""Host side of the fixed-point layered decoder (ldpc_plan_layers_q8,
ldpc_plan_qc_q8) and its numpy restatement (tests/layered_q8_ref.py): the
vectorised restatement equals the scalar one, the posteriors keep the bound
that makes int16 exact, and the plan functions give the documented bytes, fit
rule and refusals.  No GPU."""
import numpy as np
import pytest

import ldpc_ece535a as L
from ldpc_ece535a import codes

import layered_q8_ref as q8
import layered_ref as lref
import qc_cases as qc

LDS_LIMIT = 163840


def _dv(csr):
    return int(np.bincount(csr[3], minlength=csr[1]).max())


def _special(csr, fseed, B, db, llr_scale):
    y = qc.frames(csr, fseed, B, db)
    N = csr[1]
    if N >= 404:
        qc.plant_special(y)
    else:                                       # the same samples at columns a short code has
        y[::7, 3] = np.inf
        y[1::5, 10] = -np.inf
        y[2::9, 20] = np.nan
        y[3::4, 30:34] = 0.0
        y[1::8, 34:38] = -0.0
    return q8.plant_ties(y, llr_scale)


def _same(a, b):
    for k in q8.KEYS + ("llr",):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. the restatement ------------------------------------------------------------------

def test_quantise_rules():
    y = np.array([[np.inf, -np.inf, np.nan, 0.0, -0.0, -0.0625, 0.0625, -0.1875, 0.1875,
                   -15.9375, 15.9375, -0.3125, 100.0, -100.0]], np.float32)
    want = [-127, 127, 0, 0, 0, 0, 0, 2, -2, 127, -127, 2, -127, 127]   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert q8.quantise(y, 8.0)[0].tolist() == want
    assert [q8._quantise_scalar(v, 8.0, 1.0) for v in y[0]] == want
    assert q8.quantise(y, 8.0, polarity=-1.0)[0].tolist() == [-v for v in want]


@pytest.mark.parametrize("name,num,cap", [("E", 16, 20), ("E", 13, 20), ("G", 13, 6)])
def test_decode_equals_decode_scalar_on_block_rows(name, num, cap):
    base, Z = qc.base_of(name)
    csr = L.plan_qc(base, Z)["csr"]
    plan = qc.block_rows(base.shape[0], Z)
    fseed, B, db = (105, 24, 1.0) if name == "E" else (107, 12, 5.0)
    y = _special(csr, fseed, B, db, 8.0)
    ref = q8.decode(csr, plan, y, cap, num=num, llr_scale=8.0)
    _same(ref, q8.decode_scalar(csr, plan, y, cap, num=num, llr_scale=8.0))
    assert (ref["iters"] < cap).any()
    assert np.abs(ref["llr"]).max() <= 127 * (_dv(csr) + 1)
    assert (ref["llr"] == np.rint(ref["llr"])).all()


def test_decode_equals_decode_scalar_on_a_first_fit_plan():
    """A small IRA code under first fit, et_period 3, polarity -1, llr_scale 16."""
    csr = lref.ira_code(360, 720, 1)
    plan = lref.first_fit(csr)
    y = q8.plant_ties(qc.plant_special(-lref.noisy(csr, 6, 2.0, 31)), 16.0)
    kw = dict(num=13, llr_scale=16.0, et_period=3, polarity=-1.0)
    ref = q8.decode(csr, plan, y, 9, **kw)
    _same(ref, q8.decode_scalar(csr, plan, y, 9, **kw))
    assert np.abs(ref["llr"]).max() <= 127 * (_dv(csr) + 1)
    assert (ref["iters"] % 3 == 0).all()


def test_a_sample_that_quantises_to_zero_does_not_freeze():
    """sign(0) = +1: a column whose sample is 0 is moved by its rows."""
    base, Z = qc.base_of("E")
    csr = L.plan_qc(base, Z)["csr"]
    y = qc.frames(csr, 105, 8, 6.0)
    y[:, 25] = 0.0
    ref = q8.decode(csr, qc.block_rows(base.shape[0], Z), y, 20)
    assert (ref["llr"][:, 25] != 0).all()


# ---- 2. the plan functions ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F", "G"])
def test_plan_qc_q8_bytes(name):
    base, Z = qc.base_of(name)
    M, N, rp, ci = L.plan_qc(base, Z)["csr"]
    p = L.plan_qc_q8(base, Z)
    assert p["lds_bytes"] == q8.frame_bytes(N, int(rp[M])) <= LDS_LIMIT and p["fits"]
    assert p["threads"] == L.plan_qc(base, Z)["threads"] == 64 * -(-Z // 64)
    t = L.plan_layers_q8((M, N, rp, ci))
    f = L.plan_layers((M, N, rp, ci), precision=1)
    assert t["fits"] and (t["layer_of_row"] == f["layer_of_row"]).all()
    assert (t["n_layers"], t["threads"]) == (f["n_layers"], f["threads"])
    tables = q8.a16(4 * M) + q8.a16(2 * int(rp[M])) + q8.a16(2 * M) + q8.a16(4 * (t["n_layers"] + 1))
    frame = q8.frame_bytes(N, int(rp[M]))
    assert t["lds_bytes"] == (frame + tables if frame + tables <= LDS_LIMIT else frame)


def test_larger_than_float():
    base = q8.large_base(12)
    f = L.plan_qc(base, 1024, precision=L.PREC_F32)
    assert not f["fits"] and f["lds_bytes"] == 188544
    M, N, rp, ci = f["csr"]
    assert (N, int(rp[M])) == (12288, 31744)
    p = L.plan_qc_q8(base, 1024)
    assert p["fits"] and p["lds_bytes"] == 56448 and p["threads"] == 1024
    assert L.plan_layers_q8(f["csr"])["fits"]           # E <= 65535: the table route takes it too


def test_e_past_16_bits():
    base = q8.large_base(24)
    assert int((base >= 0).sum()) == 67
    f = L.plan_qc(base, 1024, precision=L.PREC_F32)
    M, N, rp, ci = f["csr"]
    assert not f["fits"] and int(rp[M]) == 68608
    p = L.plan_qc_q8(base, 1024)
    assert p["fits"] and p["lds_bytes"] == 117888
    t = L.plan_layers_q8(f["csr"])                      # refused by the table route: E
    assert not t["fits"] and t["lds_bytes"] == 117888


def test_lds_boundary():
    inside, beyond = q8.boundary_base(63), q8.boundary_base(64)
    assert not L.plan_qc(inside, 1024, precision=L.PREC_F32)["fits"]
    p = L.plan_qc_q8(inside, 1024)
    assert p["fits"] and p["lds_bytes"] == 162944 == 98304 + 64512 + 128 <= LDS_LIMIT
    p = L.plan_qc_q8(beyond, 1024)
    assert not p["fits"] and p["lds_bytes"] == 163968 > LDS_LIMIT


def test_degree_limits():
    base = np.full((2, 40), -1, np.int32)
    base[0, :33] = 0
    base[1, 30:] = 1
    p = L.plan_qc_q8(base, 4)
    assert not p["fits"] and p["lds_bytes"] == q8.frame_bytes(160, 43 * 4)
    base[0, 32] = -1
    assert L.plan_qc_q8(base, 4)["fits"]


def test_refusals():
    ok = np.array([[0, 1, -1], [-1, 2, 0]], np.int32)
    assert L.plan_qc_q8(ok, 3)["fits"]
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*Z = 0"):
        L.plan_qc_q8(np.array([[-1, -1]], np.int32), 0)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*Z = 1025"):
        L.plan_qc_q8(ok, 1025)
    with pytest.raises(L.LdpcError, match=r"LDPC_EINVAL.*\(1, 1\).*shift 3 "):
        L.plan_qc_q8(np.array([[0, 1, -1], [-1, 3, 0]], np.int32), 3)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*at least one row"):
        L.plan_qc_q8(np.zeros((0, 3), np.int32), 3)
    with pytest.raises(L.LdpcError, match="a base matrix is two-dimensional"):
        L.plan_qc_q8(np.arange(3), 3)
    M, N, rp, ci = codes.qc_expand(ok, 3)
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*CSR H"):
        L.plan_layers_q8((M, N, rp, ci[::-1].copy()))
    with pytest.raises(L.LdpcError, match="LDPC_EINVAL.*CSR H"):
        L.plan_layers_q8((N, M, rp, ci))


# ---- 3. the host-only budget and table code under the sanitizers -------------------------

def test_budget_and_tables_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/native/layers_q8_check.cc, its own main)
    built with the planning sources and -fsanitize=address,undefined."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd", "csrc")
    exe = str(tmp_path / "layers_q8_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(here, "native", "layers_q8_check.cc"),
                           os.path.join(csrc, "ldpc_layers.cc"), os.path.join(csrc, "ldpc_qc.cc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layers_q8_check ok" in out.stdout, out.stderr
