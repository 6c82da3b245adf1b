#!/usr/bin/env python3
"""A/B of the layered decodes whose frame load recovers rate-matched samples
(ldpc_decode_layered_rm_device, ldpc_decode_layered_q8_rm_device:
ldpc_layered.hip load_frame_rm) against the two-step route of the same build,
ldpc_rate_recover_device into an HBM array of (B, N) samples and then the plain
layered decode of it; and of the identity pattern through the new entry point
against the plain entry point on the same samples, which is expected to tie.

Codes: the synthetic dual diagonals of tests/qc_cases.py, "C" (Z = 96, N = 2880)
and "D" (Z = 384, N = 3840).  Patterns, as tests/rate_match_cases.py's (b) and
(c) scaled to the lifting size: "b" punctures 2 Z positions, has 40 fillers,
the full buffer and one transmission (0, S - 3 Z); "c" punctures 2 Z, has 70
fillers, a buffer cut by Z and one transmission (S - 100, S + 150), a wrap and
a repetition.  The frames are made on the device (random bits with the fillers
zeroed -> encoder -> bit selector -> BPSK + noise); unreceived columns enter at
2^-10.  B = 1, 64, 4096; f32 at scale 0.8125 and q8 at num 13.

The method is tools/layered_ab.py's: each leg times its calls plus a
synchronise, after a warm-up, for at least --seconds per round, the legs
alternating for --rounds rounds in one process on the same data.  Reported per
leg: microseconds per call as the median over rounds with the spread (max -
min).  Before the timing the two legs' outputs are asserted equal.  A leg wins
where its median beats the other's by more than three times the larger of the
two spreads.  Run on an MI355X; --out also writes the table to a file."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.environ.get("LDPC_PKG_DIR", os.path.join(REPO, "gr-ldpc_ece535a_amd")))
import torch  # noqa: E402
import ldpc_ece535a as L  # noqa: E402
from ldpc_ece535a import _capi, ber  # noqa: E402
import qc_cases as qc  # noqa: E402

UNRECEIVED = 2.0 ** -10


def patterns(N, K, Z):
    """name -> ((punct, filler, ncb), tx)."""
    sb = N - 2 * Z - 40
    sc = N - 2 * Z - Z - 70
    return {"b": ((2 * Z, 40, 0), [(0, sb - 3 * Z)]),
            "c": ((2 * Z, 70, N - 2 * Z - Z), [(sc - 100, sc + 150)]),
            "identity": ((0, 0, 0), [(0, N)])}


class Leg:
    def __init__(self, name, fn, sync):
        self.name, self.fn, self.sync = name, fn, sync

    def call(self):
        self.fn()
        self.sync()

    def timed(self, seconds):
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
    ap.add_argument("--ebn0", type=float, default=9.0)
    ap.add_argument("--cap", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.seconds < 0.5:
        ap.error("at least 3 rounds of at least 0.5 s per leg")
    lines = []
    tally = {"fused": [0, 0, 0], "identity": [0, 0, 0]}   # wins, losses, ties

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# layered decode of rate-matched samples: fused frame load vs rate_recover_device + the "
        "plain decode, %s" % torch.cuda.get_device_name(0))
    say("# synthetic base matrices; %d rounds of >= %.1f s per leg, legs alternated; median and "
        "spread (max - min) over rounds; %.1f dB, cap %d, f32 scale 0.8125, q8 num 13"
        % (args.rounds, args.seconds, args.ebn0, args.cap))
    say("# %5s %-8s %5s %-4s %-30s | %12s %10s" % ("N", "pattern", "B", "", "leg", "us/call", "spread"))
    for code in ("C", "D"):
        base, Z = qc.base_of(code)
        dec = L.Decoder(qc=(base, Z))
        N, K = dec.N, dec.K
        for pname, (pat, tx) in patterns(N, K, Z).items():
            dec.set_rate_match(*pat)
            total = sum(e for _, e in tx)
            for B in args.batches:
                d_data = torch.empty((B, K), dtype=torch.uint8, device="cuda")
                _capi.random_bits(d_data.data_ptr(), B * K, 1000 + B)
                if pat[1]:
                    d_data[:, K - pat[1]:] = 0
                torch.cuda.synchronize()
                d_cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
                d_sent = torch.empty((B, total), dtype=torch.uint8, device="cuda")
                d_rx = torch.empty((B, total), dtype=torch.float32, device="cuda")
                d_y = torch.zeros((B, N), dtype=torch.float32, device="cuda")
                dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr())
                off = 0
                for k0, e in tx:
                    dec.rate_match_device(d_cw.data_ptr(), B, k0, e, d_sent.data_ptr() + off,
                                          out_stride=total)
                    off += e
                _capi.bpsk_awgn(d_sent.data_ptr(), B * total, ber.sigma_of(args.ebn0), 7,
                                d_rx.data_ptr())
                dec.synchronize()
                torch.cuda.synchronize()
                out = [dict(pk=torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda"),
                            it=torch.zeros(B, dtype=torch.int32, device="cuda")) for _ in range(2)]
                for arith in ("f32", "q8"):
                    def fused(o=out[0]):
                        kw = dict(max_iters=args.cap, unreceived_lci=UNRECEIVED,
                                  d_iters=o["it"].data_ptr())
                        if arith == "q8":
                            dec.decode_layered_q8_rm_device(d_rx.data_ptr(), B, tx,
                                                            o["pk"].data_ptr(), num=13, **kw)
                        else:
                            dec.decode_layered_rm_device(d_rx.data_ptr(), B, tx, o["pk"].data_ptr(),
                                                         scale=0.8125, precision=L.PREC_F32, **kw)

                    def plain(o=out[1]):
                        kw = dict(max_iters=args.cap, d_iters=o["it"].data_ptr())
                        if arith == "q8":
                            dec.decode_layered_q8_device(d_y.data_ptr(), B, o["pk"].data_ptr(),
                                                         num=13, **kw)
                        else:
                            dec.decode_layered_device(d_y.data_ptr(), B, o["pk"].data_ptr(),
                                                      scale=0.8125, precision=L.PREC_F32, **kw)

                    def two_steps():
                        dec.rate_recover_device(d_rx.data_ptr(), B, tx, d_y.data_ptr(),
                                                unreceived_lci=UNRECEIVED)
                        plain()

                    if pname == "identity":
                        # the plain entry point on the recovered samples, made once
                        dec.rate_recover_device(d_rx.data_ptr(), B, tx, d_y.data_ptr(),
                                                unreceived_lci=UNRECEIVED)
                        dec.synchronize()
                        legs = [Leg("identity through _rm", fused, dec.synchronize),
                                Leg("plain entry point", plain, dec.synchronize)]
                    else:
                        legs = [Leg("fused frame load", fused, dec.synchronize),
                                Leg("rate_recover + plain decode", two_steps, dec.synchronize)]
                    for leg in legs:
                        leg.call()
                        leg.call()
                    assert torch.equal(out[0]["pk"], out[1]["pk"])
                    assert torch.equal(out[0]["it"], out[1]["it"])
                    iters = out[0]["it"].cpu().numpy()
                    t = [[] for _ in legs]
                    for _ in range(args.rounds):
                        for k, leg in enumerate(legs):
                            t[k].append(leg.timed(args.seconds))
                    med, spread = [], []
                    for k, leg in enumerate(legs):
                        us = 1e6 * np.array(t[k])
                        med.append(float(np.median(us)))
                        spread.append(float(us.max() - us.min()))
                        say("  %5d %-8s %5d %-4s %-30s | %12.1f %10.1f" % (
                            N, pname, B, arith, leg.name, med[k], spread[k]))
                    gap, need = med[1] - med[0], 3 * max(spread)
                    v = 0 if gap > need else 1 if -gap > need else 2
                    tally["identity" if pname == "identity" else "fused"][v] += 1
                    say("#   %s %s (%.2fx; gap %.1f us, three spreads %.1f us; mean iterations "
                        "%.1f, %d of %d frames at the cap)" % (
                            legs[0].name, ("wins", "loses", "ties")[v], med[1] / med[0], gap, need,
                            iters.mean(), int((iters == args.cap).sum()), B))
        dec.close()
    say("# tally, fused against two steps: %d wins, %d losses, %d ties" % tuple(tally["fused"]))
    say("# tally, identity through _rm against the plain entry point: %d wins, %d losses, %d ties"
        % tuple(tally["identity"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
