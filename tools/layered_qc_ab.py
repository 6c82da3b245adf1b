#!/usr/bin/env python3
"""A/B of the circulant layered kernel (ldpc_create_qc, ldpc_layered.hip)
against what the same build already runs on the same code: the per-edge table
kernel under the same block-row plan (LDPC_FLAG_QC_TABLES), the table kernel
under the first-fit plan (a CSR context of the expanded H), and flooding
min-sum on the on-chip path.  Codes: synthetic dual-diagonal base matrices
(codes.qc_dual_diagonal) of Z = 27 / N = 648, Z = 96 / N = 2304 and Z = 384 /
N = 3840; precision 0, 50-iteration cap, 2 dB, B = 1, 64, 4096 device-resident
frames, scales 1.0 and 0.8125.

The method is tools/layered_ab.py's: each leg times its decode call plus a
synchronise, after a warm-up, for at least --seconds per round, the legs
alternating for --rounds rounds in one process on the same frames.  Reported
per leg: microseconds per call as the median over rounds with the spread (max
- min), mean iterations and frames left with a non-zero syndrome.  Before the
timing the table kernel's outputs under the block-row plan are asserted equal
to the circulant kernel's (same contract, same plan).  A leg wins where its
median beats the other's by more than three times the larger of the two
spreads.  Run on the GPU box; --out also writes the table to a file."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ.get("LDPC_PKG_DIR", os.path.join(REPO, "gr-ldpc_ece535a_amd")))
import torch  # noqa: E402
import ldpc_ece535a as L  # noqa: E402
from ldpc_ece535a import codes  # noqa: E402

# (mb, nb, Z, info_deg, seed): synthetic base matrices
CODES = [(12, 24, 27, 3, 2), (12, 24, 96, 3, 7), (4, 10, 384, 3, 4)]
SCALES = (1.0, 0.8125)


def frames(csr, B, db, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, csr[1] - csr[0]), dtype=np.uint8)
    x = 2.0 * codes.qc_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


class Leg:
    """scale None: the context's flooding min-sum (method 0)."""

    def __init__(self, name, dec, d_y, B, iters, scale=None):
        self.name, self.dec, self.d_y, self.B, self.iters, self.scale = name, dec, d_y, B, iters, scale
        self.pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
        self.it = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.sy = torch.zeros(B, dtype=torch.int32, device="cuda")

    def call(self):
        kw = dict(max_iters=self.iters, d_iters=self.it.data_ptr(), d_synd=self.sy.data_ptr())
        if self.scale is None:
            self.dec.decode_device(self.d_y.data_ptr(), self.B, self.pk.data_ptr(), method=0, **kw)
        else:
            self.dec.decode_layered_device(self.d_y.data_ptr(), self.B, self.pk.data_ptr(),
                                           scale=self.scale, **kw)
        self.dec.synchronize()

    def outputs(self):
        return [t.cpu().numpy() for t in (self.pk, self.it, self.sy)]

    def timed(self, seconds):
        """Seconds per call over at least `seconds` of calls."""
        n, t0 = 0, time.perf_counter()
        while True:
            self.call()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return dt / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.seconds < 0.5:
        ap.error("at least 3 rounds of at least 0.5 s per leg")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# circulant layered kernel vs the table kernel and flooding min-sum, %s"
        % torch.cuda.get_device_name(0))
    say("# synthetic dual-diagonal QC codes; precision 0, cap %d, %.1f dB, %d rounds of >= %.1f s "
        "per leg, legs alternated; median and spread (max - min) over rounds"
        % (args.iters, args.ebn0, args.rounds, args.seconds))
    say("# %4s %5s %-28s | %12s %10s | %10s %8s" % (
        "N", "B", "leg", "us/call", "spread", "mean iters", "failed"))
    for mb, nb, Z, info_deg, seed in CODES:
        base = codes.qc_dual_diagonal(mb, nb, Z, info_deg, seed)
        plan = L.plan_qc(base, Z)
        csr = plan["csr"]
        M, N, E = csr[0], csr[1], csr[3].size
        dc = int(np.diff(csr[2]).max())
        dv = int(np.bincount(csr[3], minlength=N).max())
        onchip = all(L._capi.plan_onchip(M, N, E, dc, dv, method=m, precision=p)["fits"]
                     for m in (0, 1) for p in range(4))
        y = frames(csr, max(args.batches), args.ebn0, 2024 + N)
        d_y = torch.from_numpy(y).cuda()
        circ = L.Decoder(qc=(base, Z), onchip=onchip)
        tabs = L.Decoder(qc=(base, Z), qc_tables=True)
        fit = L.Decoder(csr=csr)
        assert circ.qc is not None and (circ.layers == tabs.layers).all() and fit.qc is None
        first = L.plan_layers(csr)
        say("# N = %d (mb %d, nb %d, Z %d, E %d, dc <= %d): %d block rows on %d threads, %d bytes "
            "of LDS; first fit %d layers on %d threads, %d bytes%s" % (
                N, mb, nb, Z, E, dc, mb, plan["threads"], plan["lds_bytes"], first["n_layers"],
                first["threads"], first["lds_bytes"],
                "" if onchip else "; flooding min-sum does not fit the on-chip kernels"))
        for B in args.batches:
            legs = []
            for s in SCALES:
                legs += [Leg("circulant %g" % s, circ, d_y, B, args.iters, s),
                         Leg("tables, block rows %g" % s, tabs, d_y, B, args.iters, s),
                         Leg("tables, first fit %g" % s, fit, d_y, B, args.iters, s)]
            if onchip:
                legs.append(Leg("flooding min-sum on-chip", circ, d_y, B, args.iters))
            for leg in legs:  # warm-up: code objects, tables, workspaces, queues
                leg.call()
                leg.call()
            for a in (0, 3):  # same contract, same plan: the same outputs
                for u, v in zip(legs[a].outputs(), legs[a + 1].outputs()):
                    assert (u == v).all(), "%s and %s differ" % (legs[a].name, legs[a + 1].name)
            t = [[] for _ in legs]
            for _ in range(args.rounds):
                for k, leg in enumerate(legs):
                    t[k].append(leg.timed(args.seconds))
            med, spread = [], []
            for k, leg in enumerate(legs):
                us = 1e6 * np.array(t[k])
                med.append(float(np.median(us)))
                spread.append(float(us.max() - us.min()))
                _, it, sy = leg.outputs()
                say("  %4d %5d %-28s | %12.1f %10.1f | %10.2f %8d" % (
                    N, B, leg.name, med[k], spread[k], it.mean(), int((sy != 0).sum())))
            pairs = [(0, 1), (0, 2), (3, 4), (3, 5)] + ([(0, 6), (3, 6)] if onchip else [])
            for a, b in pairs:
                gap, need = med[b] - med[a], 3 * max(spread[a], spread[b])
                verdict = "wins" if gap > need else "loses" if -gap > need else "ties"
                say("#   %s %s against %s (%.2fx; gap %.1f us, three spreads %.1f us)" % (
                    legs[a].name, verdict, legs[b].name, med[b] / med[a], gap, need))
        for d in (circ, tabs, fit):
            d.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
