"""ldpc_math_probe for the device tests: one function of the decode kernels'
arithmetic on host arrays, through device buffers with a canary behind them."""
import numpy as np
import torch

import ldpc_ece535a as L
import math_sets as ms

C = L._capi
CANARY = 16
SENTINEL = -1234.5


class Probe:
    def __init__(self):
        self.dec = L.Decoder()

    def __call__(self, fn, prec, a, b=None):
        """fn at precision prec on a (and b), padded to a multiple of three; the
        n results, the canary behind them checked"""
        dt = np.float32 if prec == C.PREC_F32 else np.float64
        div = fn >= C.PROBE_DIV1
        a = np.ascontiguousarray(a, dt).ravel()
        n0 = a.size
        a = ms.triples(a, 1.0 if div else 0.5)
        d_a = torch.from_numpy(a).cuda()
        d_b = None
        if b is not None:
            d_b = torch.from_numpy(ms.triples(np.ascontiguousarray(b, dt).ravel(),
                                              1.0 if div else 0.0)).cuda()
            assert d_b.numel() == a.size
        out = torch.full((a.size + CANARY,), SENTINEL, dtype=d_a.dtype, device="cuda")
        torch.cuda.synchronize()
        self.dec.math_probe(fn, prec, d_a.data_ptr(), a.size, out.data_ptr(),
                            d_b.data_ptr() if d_b is not None else None)
        self.dec.synchronize()
        h = out.cpu().numpy()
        assert (h[a.size:] == dt(SENTINEL)).all(), "the call wrote past its n elements"
        return h[:n0]

    def close(self):
        self.dec.close()
