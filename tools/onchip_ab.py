#!/usr/bin/env python3
"""A/B of the on-chip path (LDPC_FLAG_ONCHIP, ldpc_onchip.hip) against the
large-code path (LDPC_FLAG_GRAPH) of the same build, on the N = 720 and
N = 2160 IRA codes: min-sum and sum-product at precision 0, 50-iteration cap,
2 dB, B = 1, 64, 4096 device-resident frames.

Each leg times ldpc_decode_device plus a synchronise, after a warm-up, for at
least --seconds per round, the two contexts alternating for --rounds rounds
in one process; the outputs of the two legs (packed bytes, iterations,
syndrome weights) are compared on every round.  Reported: microseconds per
call (per frame at B = 1) and Mbit/s of information bits, as the median over
rounds with the min..max spread.  Run on the GPU box; --out also writes the
table to a file."""
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
    def __init__(self, dec, d_y, B, method, iters):
        self.dec, self.d_y, self.B, self.method, self.iters = dec, d_y, B, method, iters
        self.pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
        self.it = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.sy = torch.zeros(B, dtype=torch.int32, device="cuda")

    def call(self):
        self.dec.decode_device(self.d_y.data_ptr(), self.B, self.pk.data_ptr(),
                               method=self.method, max_iters=self.iters,
                               d_iters=self.it.data_ptr(), d_synd=self.sy.data_ptr())
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

    def outputs(self):
        return [t.cpu().numpy() for t in (self.pk, self.it, self.sy)]


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

    say("# on-chip vs large-code path, same build, %s" % torch.cuda.get_device_name(0))
    say("# precision 0, cap %d, %.1f dB, %d rounds of >= %.1f s per leg, contexts alternated; "
        "median [min..max] over rounds" % (args.iters, args.ebn0, args.rounds, args.seconds))
    say("# %4s %6s %5s | %32s | %32s | %7s %s" % ("N", "method", "B", "on-chip us/call",
                                                  "large-code us/call", "speedup", "Mbit/s on-chip "
                                                  "/ large-code (info bits)"))
    for n, kw in CODES.items():
        csr = codes.ira_from_table(codes.dvbs2_like_table(3, hi_deg=6, lo_deg=3, **kw),
                                   kw["K"], kw["N"])
        y = frames(csr, max(args.batches), args.ebn0, 2024 + n)
        d_y = torch.from_numpy(y).cuda()
        on, gr = L.Decoder(csr=csr, onchip=True), L.Decoder(csr=csr, force_graph=True)
        assert on.path == L._capi.PATH_ONCHIP and gr.path == L._capi.PATH_GRAPH
        for method in (0, 1):
            for B in args.batches:
                legs = [Leg(on, d_y, B, method, args.iters), Leg(gr, d_y, B, method, args.iters)]
                for leg in legs:  # warm-up: code objects, workspaces, queues
                    leg.call()
                    leg.call()
                t = [[], []]
                for r in range(args.rounds):
                    for k, leg in enumerate(legs):
                        t[k].append(leg.timed(args.seconds))
                    a, b = legs[0].outputs(), legs[1].outputs()
                    for name, x, z in zip(("packed", "iters", "synd"), a, b):
                        if not np.array_equal(x, z):
                            raise SystemExit("N=%d method=%d B=%d round %d: %s differ between "
                                             "the paths" % (n, method, B, r, name))
                us = [1e6 * np.array(x) for x in t]
                med = [float(np.median(x)) for x in us]
                mbit = [B * kw["K"] / m for m in med]
                say("  %4d %6s %5d | %10.1f [%9.1f..%9.1f] | %10.1f [%9.1f..%9.1f] | %6.2fx "
                    "%9.1f / %9.1f" % (n, ("min-sum", "sum-prod")[method], B, med[0],
                                       us[0].min(), us[0].max(), med[1], us[1].min(),
                                       us[1].max(), med[1] / med[0], mbit[0], mbit[1]))
        on.close()
        gr.close()
    say("# outputs (packed, iters, synd) of the two paths equal on every round")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
