#!/usr/bin/env python3
"""A/B of the layered normalized min-sum decoder (ldpc_decode_layered_device,
ldpc_layered.hip) against the min-sum routes the same build already has for a
mid-size code -- the on-chip path (LDPC_FLAG_ONCHIP) and the large-code path
(LDPC_FLAG_GRAPH) -- on the N = 720 and N = 2160 IRA codes: precision 0,
50-iteration cap, 2 dB, B = 1, 64, 4096 device-resident frames.

Legs: layered at scale 1.0, layered at scale 0.8125, flooding min-sum on-chip,
flooding min-sum on the large-code kernels.  Each leg times its decode call
plus a synchronise, after a warm-up, for at least --seconds per round, the
legs alternating for --rounds rounds in one process on the same frames.
Reported per leg: microseconds per call as the median over rounds with the
spread (max - min), mean iterations, frames left with a non-zero syndrome,
and Mbit/s of information bits.  The algorithms differ, so their outputs are
not compared here (tests/test_gpu_layered.py holds the layered kernel to its
contract); the layered legs are compared with the two flooding routes only,
never with each other: a leg wins where its median beats the other's by more
than three times the larger of the two spreads.  Run on the GPU box; --out
also writes the table to a file."""
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

CODES = {720: dict(K=360, N=720, hi_groups=1), 2160: dict(K=1080, N=2160, hi_groups=2)}


def frames(csr, B, db, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, csr[1] - csr[0]), dtype=np.uint8)
    x = 2.0 * codes.ira_encode(csr, info) - 1.0
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

    say("# layered normalized min-sum vs the build's flooding min-sum routes, %s"
        % torch.cuda.get_device_name(0))
    say("# precision 0, cap %d, %.1f dB, %d rounds of >= %.1f s per leg, legs alternated; median "
        "and spread (max - min) over rounds" % (args.iters, args.ebn0, args.rounds, args.seconds))
    say("# %4s %5s %-22s | %12s %10s | %10s %8s | %10s" % (
        "N", "B", "leg", "us/call", "spread", "mean iters", "failed", "info Mbit/s"))
    for n, kw in CODES.items():
        csr = codes.ira_from_table(codes.dvbs2_like_table(3, hi_deg=6, lo_deg=3, **kw),
                                   kw["K"], kw["N"])
        y = frames(csr, max(args.batches), args.ebn0, 2024 + n)
        d_y = torch.from_numpy(y).cuda()
        on, gr = L.Decoder(csr=csr, onchip=True), L.Decoder(csr=csr, force_graph=True)
        assert on.path == L._capi.PATH_ONCHIP and gr.path == L._capi.PATH_GRAPH
        plan = L.plan_layers(csr)
        say("# N = %d: %d layers, %d threads, %d bytes of LDS per workgroup" % (
            n, plan["n_layers"], plan["threads"], plan["lds_bytes"]))
        for B in args.batches:
            legs = [Leg("layered 1.0", on, d_y, B, args.iters, 1.0),
                    Leg("layered 0.8125", on, d_y, B, args.iters, 0.8125),
                    Leg("min-sum on-chip", on, d_y, B, args.iters),
                    Leg("min-sum large-code", gr, d_y, B, args.iters)]
            for leg in legs:  # warm-up: code objects, tables, workspaces, queues
                leg.call()
                leg.call()
            t = [[] for _ in legs]
            for _ in range(args.rounds):
                for k, leg in enumerate(legs):
                    t[k].append(leg.timed(args.seconds))
            med, spread = [], []
            for k, leg in enumerate(legs):
                us = 1e6 * np.array(t[k])
                med.append(float(np.median(us)))
                spread.append(float(us.max() - us.min()))
                it, sy = leg.it.cpu().numpy(), leg.sy.cpu().numpy()
                say("  %4d %5d %-22s | %12.1f %10.1f | %10.2f %8d | %10.1f" % (
                    n, B, leg.name, med[k], spread[k], it.mean(), int((sy != 0).sum()),
                    B * kw["K"] / med[k]))
            for a in (0, 1):
                for b in (2, 3):
                    gap, need = med[b] - med[a], 3 * max(spread[a], spread[b])
                    verdict = "wins" if gap > need else "loses" if -gap > need else "ties"
                    say("#   %s %s against %s (%.2fx; gap %.1f us, three spreads %.1f us)" % (
                        legs[a].name, verdict, legs[b].name, med[b] / med[a], gap, need))
        on.close()
        gr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
