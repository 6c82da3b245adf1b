"""CPU: the large-code path's host code (csrc/ldpc_graph_work.cc, the two
workspaces each laid out by one walk of an arena; csrc/ldpc_msn_tables.cc,
the min-sum pipeline's storage order and edge descriptors) as a program of its
own under AddressSanitizer and UBSan (tests/native/large_code_driver.cc).  The
program checks every workspace case against the totals and offsets recorded
before the layouts were rewritten; this test holds what it prints for the
tables against the library's ldpc_plan_storage_order on the same codes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import large_code_cases as lc


def _library_plan(csr, force):
    from ldpc_ece535a import _capi
    old = os.environ.get("LDPC_MSN_ORDER")
    if force is None:
        os.environ.pop("LDPC_MSN_ORDER", None)
    else:
        os.environ["LDPC_MSN_ORDER"] = force
    try:
        return _capi.plan_storage_order(csr)
    finally:
        if old is None:
            os.environ.pop("LDPC_MSN_ORDER", None)
        else:
            os.environ["LDPC_MSN_ORDER"] = old


def test_the_cases_are_what_they_say():
    shapes = {n: lc.csr_of(n) for n in lc.NAMES}
    M, N, rp, ci = shapes["reference"]
    assert (M, N, len(ci), int(np.diff(rp).max())) == (32, 64, 168, 6)   # the driver's constants
    M, N, rp, ci = shapes["ira_dc14"]
    assert M == 1800 and M % 360 == 0 and int(np.diff(rp).max()) == 14
    M, N, rp, ci = shapes["qc_m500"]
    assert M % 360 != 0 and M % 256 != 0 and N % 256 != 0


def test_host_code_under_asan_ubsan(tmp_path):
    """make large_code_asan, then the cases through the program's stdin."""
    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("no make / g++")
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "large_code_asan", "OUT=%s" % tmp_path])
    csrs = [lc.csr_of(n) for n in lc.NAMES]
    env = {k: v for k, v in os.environ.items() if k != "LDPC_MSN_ORDER"}
    out = subprocess.run([str(tmp_path / "large_code_asan")], input=lc.text(), capture_output=True,
                         text=True, env=env)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "workspaces 50 carved 36", lines[0]
    assert lines[-2:] == ["tables %d" % len(csrs), "ok"]
    body = lines[1:-2]
    assert len(body) == 3 * len(csrs) * len(lc.FORCE)
    explicit = 0
    for i, csr in enumerate(csrs):
        for j, force in enumerate(lc.FORCE):
            head, rpos, cpos = body[3 * (i * len(lc.FORCE) + j):][:3]
            w = head.split()
            assert w[:4] == ["case", str(i), "force", force or "unset"], head

            def val(key, k=1):
                return int(w[w.index(key) + k])
            score = (val("score"), val("score", 2))
            explicit += val("explicit") + val("explicit", 2)
            want = _library_plan(csr, force)
            what = "%s, LDPC_MSN_ORDER %s" % (lc.NAMES[i], force)
            assert val("order") == want["order"], what
            assert score == want["score"], what
            assert rpos.split()[0] == "rpos" and cpos.split()[0] == "cpos"
            np.testing.assert_array_equal(np.array(rpos.split()[1:], np.int32), want["rpos"], what)
            np.testing.assert_array_equal(np.array(cpos.split()[1:], np.int32), want["cpos"], what)
            rp = np.asarray(csr[2])
            assert val("rs") == int(np.diff(rp).max()), what
            assert val("cs") == int(np.bincount(csr[3], minlength=csr[1]).max()), what
    # the cases reach both orders and the explicit-list descriptors
    assert _library_plan(csrs[1], None)["order"] == 1 and _library_plan(csrs[1], "0")["order"] == 0
    assert explicit > 0
