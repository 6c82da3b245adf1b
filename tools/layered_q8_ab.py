#!/usr/bin/env python3
"""A/B of the fixed-point layered decoder (ldpc_decode_layered_q8*,
ldpc_layered.hip) against what the same build already runs on the same
code.

Codes that fit the float kernels (tools/layered_qc_ab.py's: Z = 27 / N = 648,
Z = 96 / N = 2304, Z = 384 / N = 3840): q8 against the f32 layered leg on the
same route and plan -- the circulant kernels under the block rows, the table
kernels under first fit -- at num 16 against scale 1 and num 13 against scale
0.8125.  The two codes the float kernels refuse (Z = 1024, mb = 4, nb = 12 and
24): q8 on the circulant route against flooding min-sum in f32 on an
LDPC_FLAG_GRAPH context, the only decoder such a code has without q8.
llr_scale 8, 50-iteration cap, 2 dB, B = 1, 64, 4096 device-resident frames.

The method is tools/layered_ab.py's: each leg times its decode call plus a
synchronise, after a warm-up, for at least --seconds per round, the legs
alternating for --rounds rounds in one process on the same frames.  Reported
per leg: microseconds per call as the median over rounds with the spread (max
- min), mean iterations, frames left with a non-zero syndrome, and the
workgroups a CU holds of its kernel: the least of LDS (163840 // bytes), wave
slots (32 // waves of a workgroup) and registers (4 * the compiler's waves per
SIMD for that kernel // waves of a workgroup; "-" for flooding min-sum, which
keeps no frame in LDS).  A leg wins where its median beats the other's by more
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

# (mb, nb, Z, info_deg, seed): synthetic base matrices
SMALL = [(12, 24, 27, 3, 2), (12, 24, 96, 3, 7), (4, 10, 384, 3, 4)]
LARGE = [(4, 12, 1024, 3, 32), (4, 24, 1024, 3, 44)]
PAIRS = ((16, 1.0), (13, 0.8125))
LLR_SCALE = 8.0
# waves per SIMD the compiler reports for each kernel
OCCUPANCY = {"q8 circulant": 5, "q8 tables": 7, "f32 circulant": 5, "f32 tables": 7}


def frames(csr, B, db, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    info = rng.integers(0, 2, size=(B, csr[1] - csr[0]), dtype=np.uint8)
    x = 2.0 * codes.qc_encode(csr, info) - 1.0
    return (x + np.sqrt(10 ** (-db / 10)) * rng.standard_normal(x.shape)).astype(np.float32)


def per_cu(kernel, lds_bytes, threads):
    waves = threads // 64
    return min(163840 // lds_bytes, 32 // waves, 4 * OCCUPANCY[kernel] // waves)


class Leg:
    """kind "q8" (arg: num), "f32" (arg: scale) or "flood" (the context's
    flooding min-sum in f32)."""

    def __init__(self, name, dec, d_y, B, iters, kind, arg=None, wg="-"):
        self.name, self.dec, self.d_y, self.B, self.iters = name, dec, d_y, B, iters
        self.kind, self.arg, self.wg = kind, arg, wg
        self.pk = torch.zeros((B, dec.KB), dtype=torch.uint8, device="cuda")
        self.it = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.sy = torch.zeros(B, dtype=torch.int32, device="cuda")

    def call(self):
        kw = dict(max_iters=self.iters, d_iters=self.it.data_ptr(), d_synd=self.sy.data_ptr())
        src, pk = self.d_y.data_ptr(), self.pk.data_ptr()
        if self.kind == "q8":
            self.dec.decode_layered_q8_device(src, self.B, pk, num=self.arg, llr_scale=LLR_SCALE,
                                              **kw)
        elif self.kind == "f32":
            self.dec.decode_layered_device(src, self.B, pk, scale=self.arg, precision=L.PREC_F32,
                                           **kw)
        else:
            self.dec.decode_device(src, self.B, pk, method=0, precision=L.PREC_F32, **kw)
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


def run(say, args, N, B, legs, pairs):
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
        _, it, sy = leg.outputs()
        say("  %5d %5d %-26s | %12.1f %10.1f | %10.2f %8d %6s" % (
            N, B, leg.name, med[k], spread[k], it.mean(), int((sy != 0).sum()), leg.wg))
    for a, b in pairs:
        gap, need = med[b] - med[a], 3 * max(spread[a], spread[b])
        verdict = "wins" if gap > need else "loses" if -gap > need else "ties"
        say("#   %s %s against %s (%.2fx; gap %.1f us, three spreads %.1f us)" % (
            legs[a].name, verdict, legs[b].name, med[b] / med[a], gap, need))


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

    say("# fixed-point layered min-sum (q8) vs the f32 layered kernels and flooding min-sum, %s"
        % torch.cuda.get_device_name(0))
    say("# synthetic dual-diagonal QC codes; llr_scale %g, cap %d, %.1f dB, %d rounds of >= %.1f s "
        "per leg, legs alternated; median and spread (max - min) over rounds"
        % (LLR_SCALE, args.iters, args.ebn0, args.rounds, args.seconds))
    say("# %5s %5s %-26s | %12s %10s | %10s %8s %6s" % (
        "N", "B", "leg", "us/call", "spread", "mean iters", "failed", "wg/CU"))
    for mb, nb, Z, info_deg, seed in SMALL:
        base = codes.qc_dual_diagonal(mb, nb, Z, info_deg, seed)
        f32 = L.plan_qc(base, Z, precision=L.PREC_F32)
        fix = L.plan_qc_q8(base, Z)
        csr = f32["csr"]
        N, E = csr[1], csr[3].size
        ff32, ffix = L.plan_layers(csr, precision=L.PREC_F32), L.plan_layers_q8(csr)
        y = frames(csr, max(args.batches), args.ebn0, 2024 + N)
        d_y = torch.from_numpy(y).cuda()
        circ = L.Decoder(qc=(base, Z))
        fit = L.Decoder(csr=csr)
        say("# N = %d (mb %d, nb %d, Z %d, E %d): block rows on %d threads, %d bytes of LDS in f32, "
            "%d in q8; first fit %d layers on %d threads, %d bytes in f32, %d in q8" % (
                N, mb, nb, Z, E, f32["threads"], f32["lds_bytes"], fix["lds_bytes"],
                ff32["n_layers"], ff32["threads"], ff32["lds_bytes"], ffix["lds_bytes"]))
        wg = {"q8 circulant": per_cu("q8 circulant", fix["lds_bytes"], fix["threads"]),
              "f32 circulant": per_cu("f32 circulant", f32["lds_bytes"], f32["threads"]),
              "q8 tables": per_cu("q8 tables", ffix["lds_bytes"], ffix["threads"]),
              "f32 tables": per_cu("f32 tables", ff32["lds_bytes"], ff32["threads"])}
        for B in args.batches:
            legs = []
            for num, scale in PAIRS:
                legs += [Leg("q8 circulant %d/16" % num, circ, d_y, B, args.iters, "q8", num,
                             wg["q8 circulant"]),
                         Leg("f32 circulant %g" % scale, circ, d_y, B, args.iters, "f32", scale,
                             wg["f32 circulant"]),
                         Leg("q8 first fit %d/16" % num, fit, d_y, B, args.iters, "q8", num,
                             wg["q8 tables"]),
                         Leg("f32 first fit %g" % scale, fit, d_y, B, args.iters, "f32", scale,
                             wg["f32 tables"])]
            run(say, args, N, B, legs, [(0, 1), (2, 3), (4, 5), (6, 7)])
        circ.close()
        fit.close()
    for mb, nb, Z, info_deg, seed in LARGE:
        base = codes.qc_dual_diagonal(mb, nb, Z, info_deg, seed)
        f32 = L.plan_qc(base, Z, precision=L.PREC_F32)
        fix = L.plan_qc_q8(base, Z)
        assert fix["fits"] and not f32["fits"]
        csr = f32["csr"]
        N, E = csr[1], csr[3].size
        y = frames(csr, max(args.batches), args.ebn0, 2024 + N)
        d_y = torch.from_numpy(y).cuda()
        dec = L.Decoder(qc=(base, Z), force_graph=True)
        say("# N = %d (mb %d, nb %d, Z %d, E %d): block rows on %d threads, %d bytes of LDS in q8; "
            "the f32 layered kernels refuse it (%d bytes)" % (
                N, mb, nb, Z, E, fix["threads"], fix["lds_bytes"], f32["lds_bytes"]))
        wg = per_cu("q8 circulant", fix["lds_bytes"], fix["threads"])
        for B in args.batches:
            legs = [Leg("q8 circulant %d/16" % num, dec, d_y, B, args.iters, "q8", num, wg)
                    for num, _ in PAIRS]
            legs.append(Leg("flooding min-sum f32", dec, d_y, B, args.iters, "flood"))
            run(say, args, N, B, legs, [(0, 2), (1, 2)])
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
