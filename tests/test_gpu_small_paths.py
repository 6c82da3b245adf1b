"""The three launchers of the one-wave small-code decoder on one input.

The batch kernel (csrc/ldpc_kernels.hip), the frame ring (csrc/ldpc_ring.hip)
and the window server (csrc/ldpc_serve.hip) pick their instantiation through
one dispatcher (dispatch_small, csrc/ldpc_dispatch.hpp) and differ in their
MINB policy only: the register budget a cell is built with, never its
arithmetic.  So for one code and one set of frames the three return the same
bytes: packed info bytes, iteration counts and syndrome weights (the server
publishes no iteration count).  Held here for a low-degree cell (the
reference's own H: loops of 5 / 3) and a generic one (c_32x64: NW = 1, four
slots, loops of 7 / 4), min-sum and sum-product, at both launch modes -- the
batch kernel's throughput mode is the build its MINB policy switches."""
import os

import numpy as np
import pytest

import ldpc_ece535a as L
import shape_cases as sc
from shape_cases import B, CAP, CASES, early_and_capped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_REFERENCE = {}


def _case(name):
    """(decoder, case): the reference's own H through Decoder(), or a shape case."""
    if name != "reference_h":
        c = CASES[name]
        return L.Decoder(np.array(c.H), reorder=False), c
    dec = L.Decoder()
    if "case" not in _REFERENCE:
        H = np.array(dec.H)
        _REFERENCE["case"] = sc.Case("reference_h", True, lambda: H)
    return dec, _REFERENCE["case"]


def _device_outputs(dec):
    return (torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda"),
            torch.full((B,), -1, dtype=torch.int32, device="cuda"),
            torch.full((B,), -1, dtype=torch.int32, device="cuda"))


def _host(o):
    return dict(zip(("packed", "iters", "synd"), (t.cpu().numpy() for t in o)))


@pytest.mark.parametrize("mode", [L._capi.MODE_LATENCY, L._capi.MODE_THROUGHPUT],
                         ids=["default", "throughput"])
@pytest.mark.parametrize("name,low", [("reference_h", True), ("c_32x64", False)])
def test_batch_ring_and_server_return_the_same_bytes(name, low, mode):
    dec, c = _case(name)
    s = c.shape
    assert (s["NW"], not s["generic"]) == (1, low) and (low or s["slots"] == 4), (name, s)
    assert dec.KB <= 4, name  # the server's result granules
    y = np.array(c.frames)
    N = dec.N
    d_y = torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    dec.set_launch_mode(mode)
    dec.set_schedule(1)  # the batch kernel's one-wave form, whatever the batch size
    for method in (0, 1):
        what = "%s method %d mode %d" % (name, method, mode)
        o = _device_outputs(dec)
        dec.decode_device(d_y.data_ptr(), B, o[0].data_ptr(), method=method, max_iters=CAP,
                          d_iters=o[1].data_ptr(), d_synd=o[2].data_ptr())
        dec.synchronize()
        torch.cuda.synchronize()
        batch = _host(o)
        assert early_and_capped(batch["iters"]), what

        o = _device_outputs(dec)
        torch.cuda.synchronize()
        dec.ring_begin(method=method, max_iters=CAP)
        dec.ring_wait(dec.ring_post(d_y.data_ptr(), B, o[0].data_ptr(), o[1].data_ptr(),
                                    o[2].data_ptr()))
        dec.ring_end()
        torch.cuda.synchronize()
        sc.eq(_host(o), batch, keys=("packed", "iters", "synd"), what=what + ": ring vs batch")

        # the server, one decoder workgroup per CU: a round of B windows goes one window per
        # workgroup, a round of 2 B (every frame twice) one window per wave
        win = (N * np.arange(B, dtype=np.int64)) << 1
        os.environ["LDPC_SERVE_BLOCKS_PER_CU"] = "1"
        try:
            dec.stage_span(y.ravel(), max_windows=512)
            dec.serve_begin(method=method, max_iters=CAP, max_windows=512)
            one = dec.serve_windows(win)
            two = dec.serve_windows(np.concatenate([win, win]))
            dec.serve_end()
        finally:
            os.environ.pop("LDPC_SERVE_BLOCKS_PER_CU", None)
        sc.eq(one, batch, keys=("packed", "synd"), what=what + ": server (workgroup form) vs batch")
        for half in (0, 1):
            got = {k: v[half * B:(half + 1) * B] for k, v in two.items()}
            sc.eq(got, batch, keys=("packed", "synd"), what=what + ": server (wave form) vs batch")
    dec.set_schedule(0)
    dec.set_launch_mode(L._capi.MODE_LATENCY)
    dec.close()
