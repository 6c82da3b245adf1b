#!/usr/bin/env python3
"""A/B of the quasi-cyclic device encoder (ldpc_encode_device on a context made
by ldpc_create_qc, ldpc_aux.hip k_encode_qc) against (a) the route it replaces,
a host encoder plus the copy of the codewords to the device -- codes.qc_encode
where it applies (the lower-triangular codes), and for the parity core, which
it cannot encode, the C host executor _capi.encode_qc -- (b)
the accumulator-staircase device encoder (k_encode_ira) on an IRA code of about
the same size, and (c) a fixed-point layered decode of the same batch at a
5-iteration cap, which shows the encoder's share of a BER sweep point.  Codes:
the synthetic 802.11n-shaped parity core of Z = 27 / N = 648
(codes.qc_parity_core), and the synthetic dual diagonals of Z = 96 / N = 2304
and Z = 1024 / N = 24576 (codes.qc_dual_diagonal); IRA codes of N = 720, 2160
and 24480 from seeded address tables of column degree 3.  B = 1, 64, 4096.

The method is tools/layered_ab.py's: each leg times its call plus a
synchronise, after a warm-up, for at least --seconds per round, the legs
alternating for --rounds rounds in one process on the same data.  Reported per
leg: microseconds per call as the median over rounds with the spread (max -
min).  Before the timing the device codewords are asserted equal to the host
executor's (_capi.encode_qc).  A leg wins where its median beats the other's by
more than three times the larger of the two spreads.  Run on an MI355X; --out also
writes the table to a file."""
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
from ldpc_ece535a import _capi, ber, codes  # noqa: E402

# (label, base, Z) and the IRA code (K, N) set against it
def cases():
    return [("parity core 12x24", codes.qc_parity_core(12, 0, 24, 27, 3, 21, a=1, b=0, x=6), 27,
             (360, 720)),
            ("dual diagonal 12x24", codes.qc_dual_diagonal(12, 24, 96, 3, 2), 96, (1080, 2160)),
            ("dual diagonal 4x24", codes.qc_dual_diagonal(4, 24, 1024, 3, 7), 1024, (12240, 24480))]


class Leg:
    def __init__(self, name, fn, sync):
        self.name, self.fn, self.sync = name, fn, sync

    def call(self):
        self.fn()
        self.sync()

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
    ap.add_argument("--ebn0", type=float, default=4.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.seconds < 0.5:
        ap.error("at least 3 rounds of at least 0.5 s per leg")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# quasi-cyclic device encoder vs the host route, the IRA device encoder and a cap-5 q8 "
        "layered decode, %s" % torch.cuda.get_device_name(0))
    say("# synthetic base matrices and address tables; %d rounds of >= %.1f s per leg, legs "
        "alternated; median and spread (max - min) over rounds; decode at %.1f dB, num 13"
        % (args.rounds, args.seconds, args.ebn0))
    say("# %5s %5s %-34s | %12s %10s" % ("N", "B", "leg", "us/call", "spread"))
    for label, base, Z, (ik, inn) in cases():
        plan = _capi.plan_qc_encoder(base, Z)
        dec = L.Decoder(qc=(base, Z))
        csr = codes.qc_expand(base, Z)
        ira = L.Decoder(csr=codes.ira_from_table(
            codes.dvbs2_like_table(1, K=ik, N=inn, hi_groups=0, lo_deg=3), ik, inn))
        say("# N = %d (%s, Z %d): core %d, %d levels, %d bytes of LDS; IRA code N = %d" % (
            dec.N, label, Z, plan["core"], plan["levels"], plan["lds_bytes"], inn))
        rng = np.random.Generator(np.random.PCG64(dec.N))
        for B in args.batches:
            data = rng.integers(0, 2, (B, dec.K), np.uint8)
            d_data = torch.from_numpy(data).cuda()
            d_cw = torch.zeros((B, dec.N), dtype=torch.uint8, device="cuda")
            d_host = torch.zeros((B, dec.N), dtype=torch.uint8, device="cuda")
            i_data = torch.from_numpy(rng.integers(0, 2, (B, ik), np.uint8)).cuda()
            i_cw = torch.zeros((B, inn), dtype=torch.uint8, device="cuda")
            d_tx = torch.zeros((B, dec.N), dtype=torch.float32, device="cuda")
            d_pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
            dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr())
            dec.synchronize()
            got = d_cw.cpu().numpy()
            assert (got[:min(B, 64)] == _capi.encode_qc(base, Z, data[:64])).all()
            _capi.bpsk_awgn(d_cw.data_ptr(), B * dec.N, ber.sigma_of(args.ebn0), 5, d_tx.data_ptr())
            torch.cuda.synchronize()

            if plan["core"]:
                host_name = "host encode_qc (C) + copy"

                def host():
                    d_host.copy_(torch.from_numpy(_capi.encode_qc(base, Z, data)))
            else:
                host_name = "host codes.qc_encode + copy"

                def host():
                    d_host.copy_(torch.from_numpy(codes.qc_encode(csr, data)))

            legs = [
                Leg("QC device encoder", lambda: dec.encode_device(
                    d_data.data_ptr(), B, d_cw.data_ptr()), dec.synchronize),
                Leg(host_name, host, torch.cuda.synchronize),
                Leg("IRA device encoder, N = %d" % inn, lambda: ira.encode_device(
                    i_data.data_ptr(), B, i_cw.data_ptr()), ira.synchronize),
                Leg("q8 layered decode, cap 5", lambda: dec.decode_layered_q8_device(
                    d_tx.data_ptr(), B, d_pk.data_ptr(), num=13, max_iters=5), dec.synchronize),
            ]
            for leg in legs:  # warm-up: code objects, tables, workspaces
                leg.call()
                leg.call()
            assert (d_host.cpu().numpy() == got).all()
            t = [[] for _ in legs]
            for _ in range(args.rounds):
                for k, leg in enumerate(legs):
                    t[k].append(leg.timed(args.seconds))
            med, spread = [], []
            for k, leg in enumerate(legs):
                us = 1e6 * np.array(t[k])
                med.append(float(np.median(us)))
                spread.append(float(us.max() - us.min()))
                say("  %5d %5d %-34s | %12.1f %10.1f" % (dec.N, B, leg.name, med[k], spread[k]))
            for b in (1, 2, 3):
                gap, need = med[b] - med[0], 3 * max(spread[0], spread[b])
                verdict = "wins" if gap > need else "loses" if -gap > need else "ties"
                say("#   %s %s against %s (%.2fx; gap %.1f us, three spreads %.1f us)" % (
                    legs[0].name, verdict, legs[b].name, med[b] / med[0], gap, need))
        dec.close()
        ira.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
