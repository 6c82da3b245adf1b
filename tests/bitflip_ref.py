"""numpy restatement of the reference's bit-flipping decoder, from its text
(TEST INFRASTRUCTURE ONLY).

decodeBitFlipping, lib/ldpc_decoder_cb_impl.cc:414-476 of
ericdegroot/gr-ldpc_ece535a, vectorised over frames and kept dense like the
text: E is formed for every (i, j), edge or not, and the vote masks it with
H(i, j) != 0.  It shares no code with the oracle's three restatements
(oracle/ldpc_oracle.c: bitflip_et and orc_bitflip_sparse;
oracle/ldpc_oracle_py.py: decode_bitflip), which tests/test_bitflip_ref_host.py
holds it against on codes where columns do flip (tests/bitflip_cases.py).

`mutant` switches one line of the text to a plausible wrong reading; the
host tests show that the cases' frames tell each of them from the text.
"""
import numpy as np

# one wrong reading each; see decode() for the line it replaces
MUTANTS = (
    "ge",          # disagreements >= M / 2                          (:464)
    "ceil",        # the threshold (M + 1) / 2: differs for odd M     (:464)
    "toggle",      # ci(j) = 1 - ci(j), not 1 - y(j)                  (:465)
    "reset",       # ci(j) = y(j) when the vote fails: no stickiness  (:464-466)
    "whole_row",   # E(i, j) over the whole row, column j included    (:445)
    "nonedges",    # votes counted where H(i, j) == 0 as well         (:458)
    "inplace",     # column j sees the new ci(k) of the columns k < j (:441-467)
    "late_bound",  # n + 2 < iterations: no exit at iteration cap - 1 (:470)
    "no_et",       # et_period ignored (every iteration tests)
    "le0",         # y = 0 for rx <= 0: differs on +-0.0 samples      (:426)
)
# "n + 1 <= iterations" (an exit allowed at the last iteration) is no mutant:
# the loop ends there anyway, with the same decision and the same count
EQUIVALENT = ("last_exit",)


def decode(H, rx, iterations, et_period=1, polarity=1.0, mutant=None):
    """H (M, N) 0/1, rx (B, N) samples.  Returns dict(bits (B, N) u8,
    iters (B,) i32, synd (B,) i32): the decision, the iterations executed
    and the weight of the decision's syndrome."""
    assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant
    Hi = np.asarray(H, np.int64)
    M, N = Hi.shape                                   # :420-421
    edge = Hi != 0
    rx = np.atleast_2d(np.asarray(rx, np.float32)).astype(np.float64) * float(polarity)
    B = rx.shape[0]
    # prior hard decision: 0 only where rx < 0, so NaN and -0.0 give 1 (:424-431)
    y = np.where(rx <= 0.0 if mutant == "le0" else rx < 0.0, 0, 1).astype(np.int64)
    ci = y.copy()                                     # :433
    half = (M + 1) // 2 if mutant == "ceil" else M // 2   # unsigned M / 2 (:464)
    if mutant == "no_et":
        et_period = 1
    iters = np.full(B, iterations, np.int32)
    live = np.ones(B, bool)
    for n in range(iterations):                       # :439
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        a, ya = ci[idx], y[idx]
        if mutant == "inplace":
            a = a.copy()
            rowsum = a @ Hi.T
            for j in range(N):
                E = (rowsum - Hi[:, j][None] * a[:, j][:, None]) % 2
                votes = ((E != ya[:, j][:, None]) & edge[:, j][None]).sum(1)
                new = np.where(votes > half, 1 - ya[:, j], a[:, j])
                rowsum += Hi[:, j][None] * (new - a[:, j])[:, None]
                a[:, j] = new
            ci[idx] = a
        else:
            # E(i, j): the mod-2 sum of ci(k) over k != j with H(i, k) != 0 (:441-452)
            rowsum = a @ Hi.T                                       # (b, M)
            if mutant == "whole_row":
                E = np.broadcast_to((rowsum % 2)[:, :, None], (idx.size, M, N))
            else:
                E = (rowsum[:, :, None] - Hi[None] * a[:, None, :]) % 2
            # disagreements with y(j) over the rows with H(i, j) != 0 (:455-461)
            dis = E != ya[:, None, :]
            if mutant != "nonedges":
                dis = dis & edge[None]
            votes = dis.sum(1)                                      # (b, N)
            flip = votes >= half if mutant == "ge" else votes > half   # :464
            if mutant == "toggle":
                ci[idx] = np.where(flip, 1 - a, a)
            elif mutant == "reset":
                ci[idx] = np.where(flip, 1 - ya, ya)
            else:
                ci[idx] = np.where(flip, 1 - ya, a)                 # (y(j) + 1) % 2 (:465)
        # finished?  (:470-472; et_period thins the test, 1 = the reference)
        bound = {"late_bound": n + 2 < iterations, "last_exit": n + 1 <= iterations}.get(
            mutant, n + 1 < iterations)
        if bound and (n + 1) % et_period == 0:
            ok = ((ci[idx] @ Hi.T) % 2).sum(1) == 0                 # checkFrame(ci, 0) == 0
            iters[idx[ok]] = n + 1
            live[idx[ok]] = False
    synd = ((ci @ Hi.T) % 2).sum(1).astype(np.int32)
    return dict(bits=ci.astype(np.uint8), iters=iters, synd=synd)


def hard(rx, polarity=1.0):
    """decodeHard, :559-572: the decision bit flipping starts from."""
    rx = np.atleast_2d(np.asarray(rx, np.float32)).astype(np.float64) * float(polarity)
    return np.where(rx < 0.0, 0, 1).astype(np.uint8)
