"""CPU: the code-block CRC's host entry points (ldpc_crc_bits, ldpc_plan_crc,
ldpc_crc_attach: csrc/ldpc_crc.cc, the text ldpc_set_crc builds the kernels'
weights with) against the numpy restatement (tests/crc_ref.py): the known
answers, the weights against the bitwise register, the attach, single-bit
errors and the refusals."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crc_ref as cr

MSG = np.unpackbits(np.frombuffer(b"123456789", np.uint8))


def _field(block, len):
    """The last len bits of a block, MSB first, as an integer."""
    return int("".join(str(int(v)) for v in block[-len:]), 2)


@pytest.mark.parametrize("name", sorted(cr.NAMED))
def test_known_answers(name):
    from ldpc_ece535a import _capi
    assert MSG.size == 72
    assert cr.register(*cr.NAMED[name], MSG) == cr.KNOWN[name]
    assert _capi.crc_bits(*cr.NAMED[name], MSG) == cr.KNOWN[name]
    assert _capi.CRCS[name] == cr.NAMED[name]


# the block lengths: A = len + 1, A no multiple of 32, A > 8192 among them
def _lengths(len):
    return [len + 1, len + 2, 33, 95, 284, 1000, 4096, 8193 + len]


def test_weights_xor_is_the_register():
    """2 000 seeded blocks: the XOR of the one bits' weights is the block's
    remainder, register(payload) ^ the CRC field; the payload's own weights
    give the payload's register; and the library's weights are the
    restatement's."""
    from ldpc_ece535a import _capi
    rng = np.random.Generator(np.random.PCG64(41))
    names = sorted(cr.NAMED)
    seen = set()
    for i in range(2000):
        name = names[i % 6]
        ln, poly = cr.NAMED[name]
        ls = [a for a in _lengths(ln) if a > ln]
        A = ls[(i // 6) % len(ls)] if i < 600 else int(rng.integers(ln + 1, 700))
        block = rng.integers(0, 2, A, np.uint8)
        if (name, A) not in seen:
            seen.add((name, A))
            plan = _capi.plan_crc(5, 5 + A + 3, 3, ln, poly)
            assert plan["A"] == A
            np.testing.assert_array_equal(plan["weights"], cr.weights(ln, poly, A))
        w = cr.weights(ln, poly, A)
        x = int(np.bitwise_xor.reduce(w[block == 1])) if block.any() else 0
        P = A - ln
        assert x == cr.register(ln, poly, block[:P]) ^ _field(block, ln), (name, A)
        assert x == int(cr.remainder(ln, poly, block)[0])
        px = int(np.bitwise_xor.reduce(w[:P][block[:P] == 1])) if block[:P].any() else 0
        assert px == _capi.crc_bits(ln, poly, block[:P]), (name, A)


@pytest.mark.parametrize("name", sorted(cr.NAMED))
def test_attach_passes_and_single_bit_errors_do_not(name):
    from ldpc_ece535a import _capi
    ln, poly = cr.NAMED[name]
    rng = np.random.Generator(np.random.PCG64(42))
    for A, filler in ((ln + 1, 0), (95, 4), (284, 40), (1000, 0)):
        M, K = 9, A + filler
        payload = rng.integers(0, 2, (4, A - ln), np.uint8)
        payload[3] = 0                                   # the all-zero block passes
        info = _capi.crc_attach(M, M + K, filler, ln, poly, payload)
        np.testing.assert_array_equal(info, cr.attach(ln, poly, payload, K))
        assert (info[:, A:] == 0).all() and info.shape == (4, K)
        assert (cr.remainder(ln, poly, info[:, :A]) == 0).all()
        assert (info[3] == 0).all()
        flipped = info[0, :A][None, :] ^ np.eye(A, dtype=np.uint8)
        assert (cr.remainder(ln, poly, flipped) != 0).all(), (name, A)


def test_refusals():
    from ldpc_ece535a import LdpcError, _capi
    with pytest.raises(LdpcError, match=r"LDPC_EINVAL.*len must be in \[1, 24\] \(got 0\)"):
        _capi.crc_bits(0, 0, MSG)
    with pytest.raises(LdpcError, match=r"LDPC_EINVAL.*len must be in \[1, 24\] \(got 25\)"):
        _capi.plan_crc(4, 100, 0, 25, 1)
    with pytest.raises(LdpcError, match=r"poly must be below 2\^len = 65536 \(got 65536\)"):
        _capi.plan_crc(4, 100, 0, 16, 1 << 16)
    with pytest.raises(LdpcError, match=r"poly must be below 2\^len = 64 \(got 97\)"):
        _capi.crc_bits(6, 0x61, MSG)
    with pytest.raises(LdpcError, match=r"A = K - filler = 16, len = 16"):
        _capi.plan_crc(4, 24, 4, *cr.CRC16)
    with pytest.raises(LdpcError, match=r"A = K - filler = 6, len = 24"):
        _capi.crc_attach(4, 12, 2, *cr.CRC24A, np.zeros((1, 1), np.uint8))
    assert _capi.plan_crc(4, 24, 3, *cr.CRC16)["A"] == 17


def test_host_code_under_asan_ubsan(tmp_path):
    """make crc_asan: tests/native/crc_driver.cc, a program of its own, over
    the host sources with -fsanitize=address,undefined."""
    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("no make / g++")
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "gr-ldpc_ece535a_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "crc_asan", "OUT=%s" % tmp_path])
    out = subprocess.run([str(tmp_path / "crc_asan")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "6 known answers" in out.stdout
