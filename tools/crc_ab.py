#!/usr/bin/env python3
"""A/B of the layered decodes that check the code-block CRC beside the syndrome
(ldpc_set_crc: ldpc_layered.hip crc_wave_share) against the plain layered
decode of the same build on the same samples:

  (a) report mode against the plain decode: the price of the check;
  (b) stop mode against the plain decode, at two iteration caps: time, mean
      iterations and the frames left undecoded (plain: syndrome > 0; stop:
      remainder != 0);
  (c) report mode against the plain decode followed by ldpc_crc_check_device
      on its packed output: the fused check against the second launch.

Codes: the synthetic dual diagonals of tests/qc_cases.py, "C" (Z = 96, N = 2880)
and "D" (Z = 384, N = 3840), CRC24A behind random payloads, made on the device
(random bits -> crc_attach_device -> encoder -> BPSK + noise).  B = 1, 64,
4096; f32 at scale 0.8125 and q8 at num 13.

The method is tools/rate_match_ab.py's: each leg times its calls plus a
synchronise, after a warm-up, for at least --seconds per round, the legs
alternating for --rounds rounds in one process on the same data.  Reported per
leg: microseconds per call as the median over rounds with the spread (max -
min).  Before the timing report mode's outputs are asserted equal to the plain
decode's, and its remainders to crc_check_device's.  A leg wins where its
median beats the other's by more than three times the larger of the two
spreads.  Run on an MI355X; --out also writes the table to a file."""
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

CRC = L.CRC24A


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
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--caps", type=int, nargs=2, default=[20, 50])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.seconds < 0.5:
        ap.error("at least 3 rounds of at least 0.5 s per leg")
    lines = []
    tally = {k: [0, 0, 0] for k in ("a", "b", "c")}   # wins, losses, ties of the CRC leg

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# layered decodes with the code-block CRC checked beside the syndrome vs the plain "
        "decode, %s" % torch.cuda.get_device_name(0))
    say("# synthetic base matrices, CRC24A; %d rounds of >= %.1f s per leg, legs alternated; "
        "median and spread (max - min) over rounds; %.1f dB, caps %d and %d, f32 scale 0.8125, "
        "q8 num 13" % (args.rounds, args.seconds, args.ebn0, args.caps[0], args.caps[1]))
    say("# %5s %5s %-4s %-34s | %12s %10s %8s %10s" % ("N", "B", "", "leg", "us/call", "spread",
                                                     "iters", "undecoded"))
    for code in ("C", "D"):
        base, Z = qc.base_of(code)
        dec = L.Decoder(qc=(base, Z))
        N, K = dec.N, dec.K
        for B in args.batches:
            dec.set_crc(*CRC)
            d_payload = torch.empty((B, K - CRC[0]), dtype=torch.uint8, device="cuda")
            d_data = torch.empty((B, K), dtype=torch.uint8, device="cuda")
            d_cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
            d_y = torch.empty((B, N), dtype=torch.float32, device="cuda")
            _capi.random_bits(d_payload.data_ptr(), d_payload.numel(), 2000 + B)
            dec.crc_attach_device(d_payload.data_ptr(), B, d_data.data_ptr())
            dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr())
            _capi.bpsk_awgn(d_cw.data_ptr(), B * N, ber.sigma_of(args.ebn0), 9, d_y.data_ptr())
            dec.synchronize()
            torch.cuda.synchronize()
            pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            sy = torch.zeros(B, dtype=torch.int32, device="cuda")
            rem = torch.zeros(B, dtype=torch.int32, device="cuda")
            for arith in ("f32", "q8"):
                def decode(cap):
                    kw = dict(max_iters=cap, d_iters=it.data_ptr(), d_synd=sy.data_ptr())
                    if arith == "q8":
                        dec.decode_layered_q8_device(d_y.data_ptr(), B, pk.data_ptr(), num=13, **kw)
                    else:
                        dec.decode_layered_device(d_y.data_ptr(), B, pk.data_ptr(), scale=0.8125,
                                                  precision=L.PREC_F32, **kw)

                def leg(mode, cap, check=False):
                    def call_with_mode():
                        # (setting a CRC whose weights the context already holds is host work only)
                        dec.set_crc(*(CRC if mode else (0, 0)), mode=mode or "report")
                        decode(cap)
                        if check:
                            dec.set_crc(*CRC)
                            dec.crc_check_device(pk.data_ptr(), B, rem.data_ptr())
                    name = "%s, cap %d%s" % (mode or "plain", cap, " + crc_check_device" if check else "")
                    return Leg(name, call_with_mode, dec.synchronize)

                c0, c1 = args.caps
                legs = [leg(None, c0), leg("report", c0), leg("stop", c0), leg(None, c0, check=True),
                        leg(None, c1), leg("stop", c1)]
                # report mode is the plain decode, and its remainders are the second launch's
                stats = []
                for lg in legs:
                    lg.call()
                    lg.call()
                    crc_on = not lg.name.startswith("plain")
                    r = dec.crc_results(B) if crc_on else None
                    stats.append((pk.clone(), it.clone(), sy.clone(), r, rem.clone()))
                for k in (0, 1, 2):
                    assert torch.equal(stats[0][k], stats[1][k]) and torch.equal(stats[0][k], stats[3][k])
                assert (stats[1][3] == stats[3][4].cpu().numpy().view(np.uint32)).all()
                t = [[] for _ in legs]
                for _ in range(args.rounds):
                    for k, lg in enumerate(legs):
                        t[k].append(lg.timed(args.seconds))
                med, spread = [], []
                for k, lg in enumerate(legs):
                    us = 1e6 * np.array(t[k])
                    med.append(float(np.median(us)))
                    spread.append(float(us.max() - us.min()))
                    iters = stats[k][1].cpu().numpy()
                    bad = stats[k][3] != 0 if stats[k][3] is not None else stats[k][2].cpu().numpy() > 0
                    say("  %5d %5d %-4s %-34s | %12.1f %10.1f %8.2f %10d" % (
                        N, B, arith, lg.name, med[k], spread[k], iters.mean(), int(bad.sum())))

                def verdict(what, new, old):
                    gap, need = med[old] - med[new], 3 * max(spread[new], spread[old])
                    v = 0 if gap > need else 1 if -gap > need else 2
                    tally[what][v] += 1
                    say("#   (%s) %s %s against %s (%.3fx; gap %.1f us, three spreads %.1f us)" % (
                        what, legs[new].name, ("wins", "loses", "ties")[v], legs[old].name,
                        med[old] / med[new], gap, need))
                verdict("a", 1, 0)
                verdict("b", 2, 0)
                verdict("b", 5, 4)
                verdict("c", 1, 3)
        dec.close()
    for what, text in (("a", "report mode against the plain decode"),
                       ("b", "stop mode against the plain decode"),
                       ("c", "the fused check against the plain decode + crc_check_device")):
        say("# tally (%s), %s: %d wins, %d losses, %d ties" % ((what, text) + tuple(tally[what])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
