"""The frame queue of the workgroup-per-frame kernels (csrc/ldpc_wgframe.hpp)
across families: the on-chip flooding kernels and the layered kernels of one
context take their frames from the same per-stream counters, bound and
advanced by one host statement (ldpc_capi_queues.hip bind_queue /
commit_queue).

One on-chip N = 720 context decodes the 5000-frame batch of the families'
test_more_frames_than_workgroups, far more frames than resident workgroups,
with flooding min-sum, layered f64, layered q8 and flooding sum-product
enqueued back to back without a wait in between: every launch but the first
starts from a counter the launches before it advanced.  Each result is held to
its own reference on all frames, never to a kernel: the sparse oracle,
tests/layered_ref.py, tests/layered_q8_ref.py."""
import numpy as np
import pytest

import layered_q8_ref as q8
import layered_ref as lref

pytestmark = pytest.mark.gpu

KEYS = ("packed", "iters", "synd")
B = 5000
SCALE, NUM, LLR_SCALE = 0.8125, 13, 8.0
FAMILIES = ("min-sum", "layered f64", "layered q8", "sum-product")


class _Case:
    def __init__(self):
        import ldpc_ece535a as L
        import torch
        self.csr = lref.ira_code(360, 720, 1)
        self.dec = L.Decoder(csr=self.csr, onchip=True)
        assert self.dec.path == L._capi.PATH_ONCHIP and self.dec.E == 2879
        self.plan = self.dec.layers
        self.y = lref.noisy(self.csr, B, 4.0, 8)
        self.d_y = torch.from_numpy(self.y).cuda()
        self.side = torch.cuda.Stream()
        self._refs = {}

    def refs(self, cap):
        """The four references at this cap, in FAMILIES' order, computed once."""
        if cap not in self._refs:
            from oracle import oracle as orc
            M, N, rp, ci = self.csr
            self._refs[cap] = (
                orc.decode_batch_sparse(0, rp, ci, M, N, self.y, cap, nthreads=16),
                lref.decode(self.csr, self.plan, self.y, cap, scale=SCALE),
                q8.decode(self.csr, self.plan, self.y, cap, num=NUM, llr_scale=LLR_SCALE),
                orc.decode_batch_sparse(1, rp, ci, M, N, self.y, cap, nthreads=16))
        return self._refs[cap]

    def buffers(self):
        import torch
        return dict(packed=torch.zeros((B, self.dec.KB), dtype=torch.uint8, device="cuda"),
                    iters=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                    synd=torch.full((B,), -1, dtype=torch.int32, device="cuda"))

    def enqueue(self, family, cap, stream, out):
        """One launch of the whole batch into `out`; does not wait."""
        dec = self.dec
        kw = dict(max_iters=cap, d_iters=out["iters"].data_ptr(), d_synd=out["synd"].data_ptr(),
                  stream=stream)
        d_y, pk = self.d_y.data_ptr(), out["packed"].data_ptr()
        if family == "layered f64":
            dec.decode_layered_device(d_y, B, pk, scale=SCALE, **kw)
        elif family == "layered q8":
            dec.decode_layered_q8_device(d_y, B, pk, num=NUM, llr_scale=LLR_SCALE, **kw)
        else:
            dec.decode_device(d_y, B, pk, method=1 if family == "sum-product" else 0, **kw)


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.dec.close()


@pytest.mark.parametrize("cap,two_streams", [(12, False), (12, True), (8, False)],
                         ids=["counter", "counter-two-streams", "stride"])
def test_families_share_the_queue(case, cap, two_streams):
    """cap 12: every workgroup's next frame is an add on the stream's counter;
    cap 8: a fixed stride, and the counters stay where they are.  With two
    streams the launches alternate between the context's stream and a second
    one, each with its own counter."""
    refs = case.refs(cap)
    for family, ref in zip(FAMILIES, refs):      # the batch exercises both exits of every family
        assert (ref["iters"] < cap).any() and (ref["iters"] == cap).any(), family
    streams = [None, case.side.cuda_stream] if two_streams else [None]
    import torch
    outs = [case.buffers() for _ in FAMILIES]
    torch.cuda.synchronize()                     # the fills ran on torch's stream
    for k, family in enumerate(FAMILIES):        # no wait between the launches
        case.enqueue(family, cap, streams[k % len(streams)], outs[k])
    case.side.synchronize()
    case.dec.synchronize()
    for family, out, ref in zip(FAMILIES, outs, refs):
        for k in KEYS:
            np.testing.assert_array_equal(out[k].cpu().numpy(), ref[k],
                                          err_msg="%s: %s at cap %d" % (family, k, cap))
