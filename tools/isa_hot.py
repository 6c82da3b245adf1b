#!/usr/bin/env python3
"""VALU issue mix of a kernel's iteration loop, hot path only, from a
`hipcc --cuda-device-only -S` listing.

Regions the wave enters only for rare lanes (bodies of branches whose first
instructions carry the ;ldpc_cold marker that LDPC_EX_COLD() emits, see
csrc/ldpc_exact.hpp) are skipped.  Each instruction is weighted by its
measured issue cost on gfx950 (tools/ubench_valu.hip, tools/ubench_f64.hip,
profiles/round3/ubench_valu.txt, 4 waves per SIMD): 4.31 cycles for f64
add/mul/fma and for any VOP3-encoded or 64-bit instruction (compares, e64
selects, 64-bit moves and shifts, converts, min/max), 2.75 for VOP1/VOP2
32-bit ones, 16.3 for v_rcp_f64.  Prints the per-iteration totals and the
mean weight of the instructions the PMC counts as "other VALU" (everything
but SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64), which bench.py's roofline uses.

A loop that tests its exit in mid-body has several backward branches: the
compiler sends each exit through a latch block in front of the header, and
only the path that goes round again branches back from the body's end.  These
are one loop: it is followed to its last backward branch and reported whole,
and the part behind the last mid-body exit branch (what a last iteration does
not execute) is reported as a figure of its own.

usage: tools/isa_hot.py <file.s> <kernel-regex> [--loop-rank K] [--json out --key K]
"""
import argparse
import collections
import json
import re

W_F64, W_VOP3, W_VOP2, W_TRANS = 4.31, 4.31, 2.75, 16.3


def weight(op):
    if "rcp_f64" in op or "rsq_f64" in op or "sqrt_f64" in op:
        return W_TRANS
    if "f64" in op or "_e64" in op or "b64" in op or "u64" in op or "i64" in op:
        return W_VOP3
    if op.startswith(("v_mad", "v_fma", "v_lshl_add", "v_add3", "v_and_or", "v_or3", "v_xor3",
                      "v_bfe", "v_bfi", "v_alignbit", "v_perm", "v_mbcnt", "v_readlane",
                      "v_writelane", "v_cndmask_b32_e64", "v_med3", "v_min3", "v_max3",
                      "v_lshl_or", "v_ldexp")):
        return W_VOP3
    return W_VOP2


def pmc_class(op):
    for k in ("add_f64", "mul_f64", "fma_f64", "fmac_f64"):
        if op.startswith("v_" + k):
            return "f64"
    if "rcp_f64" in op:
        return "trans"
    return "other"


def loops(lines):
    """(first line, last backward branch, mid-body exit branches) of every
    loop, by the block comments of the listing: a loop's blocks are its
    header (".. Loop Header") and the labels marked "in Loop: Header=<it>".
    Its backward branches are those from one of its blocks to the header or
    to a block in front of it (the latches).  A backward branch before the
    last one is an exit taken in mid-body when its target is another block
    than the last one's (the latch that leaves the loop); to the same block
    it is one more way round."""
    labels, owner, headers = {}, {}, set()
    for i, l in enumerate(lines):
        m = re.match(r"^(\.L(BB\d+_\d+)):(.*)", l)
        if not m:
            continue
        labels[m.group(1)] = i
        nxt = lines[i + 1] if i + 1 < len(lines) else ""
        h = re.search(r"in Loop: Header=(BB\d+_\d+)", m.group(3))
        if "Loop Header" in m.group(3) or "Loop Header" in nxt:
            headers.add(m.group(2))
            owner[i] = m.group(2)
        elif h:
            owner[i] = h.group(1)
    marks = sorted(labels.values())
    out = []
    for hd in headers:
        hi_ = labels[".L" + hd]
        lo = min(i for i, o in owner.items() if o == hd and i <= hi_)
        br = []
        for i, l in enumerate(lines):
            m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
            if not m or i < hi_ or not lo <= labels.get(m.group(1), -1) <= hi_:
                continue
            blk = max((x for x in marks if x <= i), default=-1)
            if owner.get(blk) == hd:
                br.append((i, labels[m.group(1)]))
        if br:
            hi, back = br[-1]
            out.append((lo, hi, [i for i, t in br[:-1] if t != back]))
    return sorted(out)


def hot_path(lines, full=False):
    hot, i = [], 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m:
            tgt = m.group(1) + ":"
            # cold: the marker sits in the first basic block the branch skips
            # (the compiler may schedule instructions of that block ahead of
            # it, but not move it into another block)
            cold, j = False, i + 1
            while j < len(lines) and not re.match(r"^\.LBB\d+_\d+:", lines[j]):
                if "ldpc_cold" in lines[j]:
                    cold = True
                    break
                j += 1
            if cold:
                k = i + 1
                while k < len(lines) and not lines[k].startswith(tgt):
                    k += 1
                if k < len(lines):  # (a backward target is no skipped region)
                    i = k
                    continue
        hot.append(l)
        i += 1
    keep = [l for l in hot if l and not l.startswith((".", ";")) and not re.match(r"^\S+:", l)]
    return keep if full else [l.split()[0] for l in keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--loop-rank", type=int, default=0,
                    help="0: the loop with the most VALU that is not the frame loop")
    ap.add_argument("--json", default=None)
    ap.add_argument("--key", default=None)
    ap.add_argument("--dump", default=None, help="write the hot path's instructions here")
    a = ap.parse_args()
    s = open(a.asm).read()
    m = re.search(r"^(\S*%s\S*):" % a.kernel, s, re.M)
    body = s[m.end():s.index(".Lfunc_end", m.end())]
    lines = [l.strip() for l in body.split("\n")]
    cand = []
    for lo, hi, exits in loops(lines):
        ins = hot_path(lines[lo:hi])
        cand.append((sum(1 for x in ins if x.startswith("v_")), lo, hi, ins, exits))
    # the iteration loops are the ones nested in the frame loop: skip loops
    # that contain another loop of real size (>= 100 VALU)
    inner = [c for c in cand
             if not any(o[1] >= c[1] and o[2] <= c[2] and o != c and o[0] >= 100
                        for o in cand)]
    inner.sort(key=lambda c: -c[0])
    n, lo, hi, ins, exits = inner[min(a.loop_rank, len(inner) - 1)]
    if a.dump:
        open(a.dump, "w").write("\n".join(hot_path(lines[lo:hi], full=True)) + "\n")

    def mix(ops):
        c = collections.Counter(x for x in ops if x.startswith("v_"))
        cyc = {"f64": 0.0, "trans": 0.0, "other": 0.0}
        cnt = {"f64": 0, "trans": 0, "other": 0}
        for op, k in c.items():
            cl = pmc_class(op)
            cyc[cl] += k * weight(op)
            cnt[cl] += k
        return c, cyc, cnt

    c, cyc, cnt = mix(ins)
    total = sum(cyc.values())
    w_other = cyc["other"] / max(1, cnt["other"])
    print("%s lines %d-%d: hot-path VALU %d (f64 add/mul/fma %d, trans %d, other %d), "
          "%.0f issue cycles per iteration; mean 'other' weight %.3f"
          % (m.group(1)[:60], lo, hi, n, cnt["f64"], cnt["trans"], cnt["other"], total, w_other))
    tail = None
    if exits:  # the part a last iteration skips: behind the last mid-body exit
        t_ins = hot_path(lines[exits[-1] + 1:hi])
        _, t_cyc, t_cnt = mix(t_ins)
        tail = {"valu": sum(t_cnt.values()), "f64": t_cnt["f64"], "trans": t_cnt["trans"],
                "other": t_cnt["other"], "issue_cycles": round(sum(t_cyc.values()), 1)}
        print("  after the exit test (lines %d-%d): VALU %d (f64 add/mul/fma %d, trans %d, other %d), "
              "%.0f issue cycles, %.3f of the iteration"
              % (exits[-1] + 1, hi, tail["valu"], tail["f64"], tail["trans"], tail["other"],
                 tail["issue_cycles"], tail["issue_cycles"] / total))
    for op, k in sorted(c.items(), key=lambda kv: -kv[1] * weight(kv[0]))[:25]:
        print("  %4d x %-26s %6.0f cycles" % (k, op, k * weight(op)))
    if a.json and a.key:
        try:
            allj = json.load(open(a.json))
        except (OSError, ValueError):
            allj = {}
        e = allj.setdefault(a.key, {})
        e["isa_hot"] = {"valu": n, "f64": cnt["f64"], "trans": cnt["trans"], "other": cnt["other"],
                        "issue_cycles_per_iteration": round(total, 1),
                        "other_weight": round(w_other, 3),
                        **({"after_exit_test": tail} if tail else {}),
                        "weights": "f64 add/mul/fma and VOP3/64-bit %g, VOP1/VOP2 %g, v_rcp_f64 %g"
                                   % (W_F64, W_VOP2, W_TRANS)}
        json.dump(allj, open(a.json, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
