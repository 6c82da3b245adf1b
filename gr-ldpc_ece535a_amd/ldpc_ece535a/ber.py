"""BER / FER sweep on the GPU.

The reference's BER program (apps/ldpc_lapack.cpp:533-811) draws random
source bits, encodes them, BPSK-modulates (2u - 1), adds white Gaussian noise
with sqrt(N0), N0 = 1 / 10^(EbN0/10) (:629-636), and decodes every frame with
four decoders -- hard BPSK, BitFlip, LogDomainSimple (min-sum) and
SumProduct, 5 iterations -- over Eb/N0 = -7 .. 10 dB in 0.5 dB steps, 30
frames per point.  Per point it reports BER = mean over frames of the
fraction of codeword bits in error (biterr, :508-517) and FER = the number of
frames whose decision fails the parity checks (checkMessage, :519-529).  It
prints an Octave script.

Here every step runs on the device through the C ABI: ldpc_random_bits ->
ldpc_encode_device -> ldpc_bpsk_awgn -> ldpc_decode_device (each method) ->
ldpc_count_bit_errors, with the syndrome weight from the decoder.  The "BPSK"
curve uses the decoder's hard method (decodeHard, which maps an exact 0.0 to
1 where the app's decodeBPSK maps it to 0 -- a probability-zero event).
The decoders are the block's (lib/ldpc_decoder_cb_impl.cc), not the app's
private copies.

    python -m ldpc_ece535a.ber [--frames 30] [--iterations 5]
                               [--ebn0 -7:10:0.5] [--code default|dvbs2] [--json out]
                               [--qc MC,ME,NB,Z,DEG,SEED | --qc dual:MB,NB,Z,DEG,SEED]
                               [--layered SCALE] [--layered-q8 NUM[:LLR_SCALE]]
                               [--rate-match PUNCT,FILLER,NCB --tx K0:E[,K0:E...]
                                [--unreceived-lci LCI]]
                               [--crc NAME[:stop]]

--qc sweeps a quasi-cyclic code in place of --code: codes.qc_parity_core (a
dual-diagonal core of MC block rows and ME extension rows, the 802.11n /
802.16e / 5G-NR parity shape) or, with "dual:", codes.qc_dual_diagonal, NB block
columns lifted by Z, information columns of degree DEG, drawn from SEED.  The
decoder is Decoder(qc=...), so the frames are encoded by the quasi-cyclic
device encoder and the layered curves run the circulant kernel.  The base
matrices are synthetic, and the JSON's "code" field says so.

--layered SCALE adds a fifth curve, "LayeredMinSum": the layered normalized
min-sum decoder (ldpc_decode_layered_device) at that scale, same iteration
cap.  --layered-q8 NUM[:LLR_SCALE] adds "LayeredMinSumQ8": its fixed-point
variant (ldpc_decode_layered_q8_device) at factor NUM / 16, the samples scaled
by LLR_SCALE (default 8) before they are rounded.  Neither is one of the
reference's decoders; without the options the output is the reference
program's four curves.

--rate-match PUNCT,FILLER,NCB with --tx K0:E[,K0:E...] sweeps the code as it is
sent (include/ldpc_hip.h, "Rate matching"): the last FILLER information bits
are zeroed before the encoder, the codewords go through ldpc_rate_match_device
once per transmission (up to four), every transmitted sample gets noise of its
own, the layered curves decode what was received with the fused entry points
(ldpc_decode_layered*_rm_device) and the reference's four decoders take the
output of ldpc_rate_recover_device.  BER is still counted over all N codeword
bits, the unsent ones included, and sigma_of keeps the reference's noise
convention: sqrt(N0) from Eb/N0 alone, with no code-rate term, so a point of a
rate-matched sweep is not the Eb/N0 of the code as sent.  The JSON says both.
--unreceived-lci is what a column no sample reaches enters the decoders with
(default 2^-100, the binding's).

--crc NAME[:stop] (CRC24A, CRC24B, CRC24C, CRC16, CRC11, CRC6) puts a code-block
CRC behind random payloads before the encoder (ldpc_crc_attach_device: the
block is the information bits in front of the fillers) and sets it on the
context (ldpc_set_crc), so the layered curves check it where they evaluate the
syndrome -- with ":stop" they also leave on a zero remainder -- and the other
decoders' packed outputs go through ldpc_crc_check_device.  Per Eb/N0 every
curve then also reports the frames that passed, the undetected errors among
them (a pass with a wrong payload) and the mean iterations, in a table of
comment lines behind the Octave script and in the JSON ("crc_pass",
"crc_undetected", "iters").
"""
import argparse
import json
import math
import sys

import numpy as np

from . import _capi

DEFAULT_EBN0 = [-7.0 + 0.5 * i for i in range(35)]  # :540
METHODS = (("BPSK", _capi.METHOD_HARD), ("BitFlip", _capi.METHOD_BITFLIP),
           ("LogDomainSimple", _capi.METHOD_LOGDOMAIN), ("SumProduct", _capi.METHOD_SUMPRODUCT))
LAYERED = "LayeredMinSum"
LAYERED_Q8 = "LayeredMinSumQ8"


def sigma_of(ebn0_db):
    """sqrt(N0), N0 = 1 / exp(EbN0 ln(10) / 10) (apps/ldpc_lapack.cpp:629)."""
    return math.sqrt(1.0 / math.exp(ebn0_db * math.log(10.0) / 10.0))


RATE_MATCH_NOTE = ("BER over all N codeword bits, the unsent ones included; sigma = sqrt(N0) from "
                   "Eb/N0 alone (the reference's convention): no code-rate term")


def sweep(dec=None, ebn0=DEFAULT_EBN0, frames=30, iterations=5, seed=0, precision=0, device=0,
          layered_scale=None, layered_q8=None, rate_match=None, tx=None,
          unreceived_lci=_capi.UNRECEIVED_LCI, crc=None):
    """Returns {method name: {"ber": [...], "fer": [...]}} over `ebn0`; with
    layered_scale also LAYERED, the layered min-sum decoder at that scale; with
    layered_q8 = (num, llr_scale) also LAYERED_Q8, the fixed-point one.  With
    rate_match = (punct, filler, ncb) and tx = [(k0, E), ...] the frames are sent
    rate-matched (see the module's docstring), a column no sample reaches
    entering every decoder with unreceived_lci.  With crc = (len, poly, stop)
    the payloads carry that CRC and every curve also has "crc_pass",
    "crc_undetected" and "iters" (see the module's docstring)."""
    import torch
    if dec is None:
        dec = _capi.Decoder(device=device)
    dev = torch.device("cuda", device)
    B, N, K = int(frames), dec.N, dec.K
    d_data = torch.empty((B, K), dtype=torch.uint8, device=dev)
    d_cw = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_tx = torch.empty((B, N), dtype=torch.float32, device=dev)
    d_bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_packed = torch.empty((B, dec.KB), dtype=torch.uint8, device=dev)
    d_synd = torch.empty(B, dtype=torch.int32, device=dev)
    d_err = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    if rate_match is not None:
        if not tx:
            raise ValueError("rate_match needs tx = [(k0, E), ...]")
        dec.set_rate_match(*rate_match)
        filler, total = int(rate_match[1]), sum(int(e) for _, e in tx)
        d_sent = torch.empty((B, total), dtype=torch.uint8, device=dev)
        d_rx = torch.empty((B, total), dtype=torch.float32, device=dev)
    filler = int(rate_match[1]) if rate_match is not None else 0
    if crc is not None:
        dec.set_crc(crc[0], crc[1], mode="stop" if crc[2] else "report")
        P = K - filler - crc[0]
        d_payload = torch.empty((B, P), dtype=torch.uint8, device=dev)
        d_rem = torch.empty(B, dtype=torch.int32, device=dev)
        d_iters = torch.empty(B, dtype=torch.int32, device=dev)
    runs = (list(METHODS) + ([(LAYERED, None)] if layered_scale is not None else []) +
            ([(LAYERED_Q8, None)] if layered_q8 is not None else []))
    out = {name: {"ber": [], "fer": []} for name, _ in runs}
    if crc is not None:
        for r in out.values():
            r.update(crc_pass=[], crc_undetected=[], iters=[])
    for i, db in enumerate(ebn0):
        s0 = (int(seed) * 1000003 + i) & 0xFFFFFFFF
        if crc is not None:
            _capi.random_bits(d_payload.data_ptr(), B * P, s0, sp)
            dec.crc_attach_device(d_payload.data_ptr(), B, d_data.data_ptr(), sp)
        else:
            _capi.random_bits(d_data.data_ptr(), B * K, s0, sp)
            if filler:
                with torch.cuda.stream(stream):
                    d_data[:, K - filler:] = 0
        dec.encode_device(d_data.data_ptr(), B, d_cw.data_ptr(), sp)
        if rate_match is None:
            _capi.bpsk_awgn(d_cw.data_ptr(), B * N, sigma_of(db), s0 ^ 0x5DEECE66D,
                            d_tx.data_ptr(), sp)
        else:
            off = 0
            for k0, e in tx:
                dec.rate_match_device(d_cw.data_ptr(), B, k0, e, d_sent.data_ptr() + off,
                                      out_stride=total, stream=sp)
                off += int(e)
            # one draw per transmitted sample: every transmission has its own noise
            _capi.bpsk_awgn(d_sent.data_ptr(), B * total, sigma_of(db), s0 ^ 0x5DEECE66D,
                            d_rx.data_ptr(), sp)
            # what the reference's decoders take: the combined samples, in column order
            dec.rate_recover_device(d_rx.data_ptr(), B, tx, d_tx.data_ptr(),
                                    unreceived_lci=unreceived_lci, stream=sp)
        for name, m in runs:
            kw = dict(max_iters=iterations, precision=precision, d_bits=d_bits.data_ptr(),
                      d_synd=d_synd.data_ptr(), stream=sp)
            if crc is not None:
                kw["d_iters"] = d_iters.data_ptr()
                with torch.cuda.stream(stream):
                    d_iters.zero_()     # a decoder without iterations leaves it
            if rate_match is not None and name == LAYERED_Q8:
                del kw["precision"]
                dec.decode_layered_q8_rm_device(d_rx.data_ptr(), B, tx, d_packed.data_ptr(),
                                                num=layered_q8[0], llr_scale=layered_q8[1],
                                                unreceived_lci=unreceived_lci, **kw)
            elif rate_match is not None and m is None:
                dec.decode_layered_rm_device(d_rx.data_ptr(), B, tx, d_packed.data_ptr(),
                                             scale=layered_scale, unreceived_lci=unreceived_lci,
                                             **kw)
            elif name == LAYERED_Q8:
                del kw["precision"]
                dec.decode_layered_q8_device(d_tx.data_ptr(), B, d_packed.data_ptr(),
                                             num=layered_q8[0], llr_scale=layered_q8[1], **kw)
            elif m is None:
                dec.decode_layered_device(d_tx.data_ptr(), B, d_packed.data_ptr(),
                                          scale=layered_scale, **kw)
            else:
                dec.decode_device(d_tx.data_ptr(), B, d_packed.data_ptr(), method=m, **kw)
            _capi.count_bit_errors(d_bits.data_ptr(), d_cw.data_ptr(), N, B, d_err.data_ptr(), sp)
            stream.synchronize()
            err = d_err.cpu().numpy().astype(np.float64)
            synd = d_synd.cpu().numpy()
            out[name]["ber"].append(float((err / N).mean()) if B else 0.0)
            out[name]["fer"].append(int((synd > 0).sum()))
            if crc is not None:
                if m is None:   # the layered decodes filled the context's array
                    rem = dec.crc_results(B)
                else:
                    dec.crc_check_device(d_packed.data_ptr(), B, d_rem.data_ptr(), sp)
                    stream.synchronize()
                    rem = d_rem.cpu().numpy().view(np.uint32)
                with torch.cuda.stream(stream):
                    wrong = (d_bits[:, N - K:N - K + P] != d_payload).any(dim=1)
                stream.synchronize()
                ok = rem == 0
                out[name]["crc_pass"].append(int(ok.sum()))
                out[name]["crc_undetected"].append(int((ok & wrong.cpu().numpy()).sum()))
                out[name]["iters"].append(float(d_iters.cpu().numpy().mean()) if B else 0.0)
    return out


def qc_code(spec):
    """(base, Z, label) of a --qc argument: "MC,ME,NB,Z,DEG,SEED"
    (codes.qc_parity_core) or "dual:MB,NB,Z,DEG,SEED" (codes.qc_dual_diagonal)."""
    from . import codes
    kind, _, nums = spec.rpartition(":")
    try:
        v = [int(x) for x in nums.split(",")]
    except ValueError:
        v = []
    if kind == "dual" and len(v) == 5:
        base, Z = codes.qc_dual_diagonal(*v), v[2]
        label = "QC dual-diagonal mb=%d nb=%d Z=%d deg=%d seed=%d" % tuple(v)
    elif kind == "" and len(v) == 6:
        base, Z = codes.qc_parity_core(*v), v[3]
        label = "QC parity-core mc=%d me=%d nb=%d Z=%d deg=%d seed=%d" % tuple(v)
    else:
        raise ValueError("--qc takes MC,ME,NB,Z,DEG,SEED or dual:MB,NB,Z,DEG,SEED")
    return base, Z, label + " (synthetic base matrix)"


def octave(ebn0, res):
    """The reference program's Octave output (apps/ldpc_lapack.cpp:707-811)."""
    f = lambda v: "%.4g" % v  # noqa: E731  (std::cout.precision(4))
    lines = ["EbN0=[" + " ".join(f(x) for x in ebn0) + " ];", "figure(1);"]
    styles = ["'or--'", "'og-'", "'ob-'", "'om-'", "'ok-'", "'oc-'"]
    names = [name for name, _ in METHODS] + [n for n in (LAYERED, LAYERED_Q8) if n in res]
    legend = "legend(" + ", ".join("'%s'" % n for n in names) + ");"
    for k, name in enumerate(names):
        lines.append("ber%d=[" % k + " ".join(f(x) for x in res[name]["ber"]) + " ];")
        lines.append("plot(EbN0, ber%d, %s);" % (k, styles[k]))
        if k == 0:
            lines.append("hold;")
    lines += ["grid on;", "hold off;", "title('Bit Error Rate');",
              legend, "xlabel('EbN0');", "ylabel('BER');", "figure(2);"]
    fstyles = ["'or:'", "'og-'", "'ob-'", "'om-'", "'ok-'", "'oc-'"]
    for k, name in enumerate(names):
        lines.append("fer%d=[" % k)
        lines.append(", ".join(str(x) for x in res[name]["fer"]))  # printVector, :71-81
        lines.append("];")
        lines.append("plot(EbN0, fer%d, %s);" % (k, fstyles[k]))
        if k == 0:
            lines.append("hold;")
    lines += ["grid on;", "hold off;", "title('Frame Errors');",
              legend, "xlabel('EbN0');", "ylabel('FER');"]
    return "\n".join(lines) + "\n"


def crc_table(ebn0, res):
    """The CRC figures as Octave comment lines: per curve and Eb/N0 the frames
    that passed, the undetected errors among them, the mean iterations."""
    lines = ["% CRC: frames passed / undetected errors / mean iterations"]
    for name, r in res.items():
        if "crc_pass" not in r:
            continue
        lines.append("% " + name)
        for db, p, u, it in zip(ebn0, r["crc_pass"], r["crc_undetected"], r["iters"]):
            lines.append("%%   %6.2f dB  %6d %6d %8.2f" % (db, p, u, it))
    return "\n".join(lines) + "\n"


def parse_range(text):
    """'a:b:step' (inclusive) or a comma list."""
    if ":" in text:
        a, b, st = (float(x) for x in text.split(":"))
        n = int(round((b - a) / st)) + 1
        return [a + st * i for i in range(n)]
    return [float(x) for x in text.split(",")]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="ldpc_ber", description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--ebn0", default="-7:10:0.5")
    ap.add_argument("--code", choices=["default", "dvbs2"], default="default")
    ap.add_argument("--qc", default=None, metavar="MC,ME,NB,Z,DEG,SEED",
                    help="a synthetic quasi-cyclic code in place of --code: a parity core of MC "
                         "block rows and ME extension rows (or dual:MB,NB,Z,DEG,SEED, the "
                         "lower-triangular dual diagonal)")
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--layered", type=float, default=None, metavar="SCALE",
                    help="add the layered normalized min-sum decoder at this scale (0 < SCALE <= 1)")
    ap.add_argument("--layered-q8", default=None, metavar="NUM[:LLR_SCALE]",
                    help="add the fixed-point layered min-sum decoder at factor NUM / 16 "
                         "(NUM in 1..16), samples scaled by LLR_SCALE (default 8)")
    ap.add_argument("--rate-match", default=None, metavar="PUNCT,FILLER,NCB",
                    help="send the code rate-matched: PUNCT leading positions never sent, FILLER "
                         "known-zero information bits, a circular buffer of NCB positions (0: "
                         "to the end); needs --tx")
    ap.add_argument("--tx", default=None, metavar="K0:E[,K0:E...]",
                    help="the transmissions of a rate-matched frame (up to four): E samples "
                         "from buffer offset K0 each, combined by the receiver")
    ap.add_argument("--unreceived-lci", type=float, default=_capi.UNRECEIVED_LCI, metavar="LCI",
                    help="with --rate-match: the Lci of a column no sample reaches (default "
                         "2^-100; 2^-10 keeps the float decoders' later iterations alive, see "
                         "DESIGN section 7f)")
    ap.add_argument("--crc", default=None, metavar="NAME[:stop]",
                    help="attach this code-block CRC (%s) to random payloads and check it in "
                         "every decode; ':stop': the layered decoders also leave on a zero "
                         "remainder" % ", ".join(sorted(_capi.CRCS)))
    a = ap.parse_args(argv)
    crc = None
    if a.crc is not None:
        cname, _, cmode = a.crc.partition(":")
        if cname not in _capi.CRCS or cmode not in ("", "stop"):
            ap.error("--crc takes NAME[:stop], NAME one of " + ", ".join(sorted(_capi.CRCS)))
        crc = _capi.CRCS[cname] + (cmode == "stop",)
    rate_match = tx = None
    if (a.rate_match is None) != (a.tx is None):
        ap.error("--rate-match and --tx go together")
    if a.rate_match is not None:
        try:
            rate_match = tuple(int(x) for x in a.rate_match.split(","))
            tx = [tuple(int(x) for x in t.split(":")) for t in a.tx.split(",")]
            if len(rate_match) != 3 or any(len(t) != 2 for t in tx):
                raise ValueError
        except ValueError:
            ap.error("--rate-match takes PUNCT,FILLER,NCB and --tx K0:E[,K0:E...]")
    q8 = None
    if a.layered_q8 is not None:
        num, _, sc = a.layered_q8.partition(":")
        q8 = (int(num), float(sc) if sc else 8.0)
    # torch first: it then shares its HIP runtime with libldpc_hip.so (see
    # INTEGRATION.md, "One HIP runtime per process")
    import torch  # noqa: F401
    code = a.code
    if a.qc is not None:
        try:
            base, Z, code = qc_code(a.qc)
        except ValueError as e:
            ap.error(str(e))
        dec = _capi.Decoder(qc=(base, Z))
    elif a.code == "dvbs2":
        from . import codes
        dec = _capi.Decoder(csr=codes.dvbs2_like(0))
    else:
        dec = _capi.Decoder()
    grid = parse_range(a.ebn0)
    res = sweep(dec, grid, a.frames, a.iterations, a.seed, a.precision, layered_scale=a.layered,
                layered_q8=q8, rate_match=rate_match, tx=tx, unreceived_lci=a.unreceived_lci,
                crc=crc)
    sys.stdout.write(octave(grid, res))
    if crc is not None:
        sys.stdout.write(crc_table(grid, res))
    if a.json:
        doc = {"ebn0": grid, "frames": a.frames, "iterations": a.iterations, "code": code,
               "results": res}
        if rate_match is not None:
            doc["rate_match"] = {"punct": rate_match[0], "filler": rate_match[1],
                                 "ncb": rate_match[2], "tx": [list(t) for t in tx],
                                 "unreceived_lci": a.unreceived_lci,
                                 "note": RATE_MATCH_NOTE}
        if crc is not None:
            doc["crc"] = {"name": a.crc.partition(":")[0], "len": crc[0], "poly": crc[1],
                          "mode": "stop" if crc[2] else "report"}
        json.dump(doc, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
