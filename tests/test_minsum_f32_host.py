"""The float contract of min-sum, checked without a GPU.

tests/minsum_ref.py restates the reference's min-sum in numpy, generic over
the arithmetic type.  Here it is pinned from both sides: at float64 it equals
the C oracle the exact modes are held to (so it states the reference's
operations in the reference's order, and cannot later be bent to fit a
kernel), at float32 it equals the oracle's own float restatement
(oracle.decode_batch(..., real="f32")), written separately in C.

The GPU tests hold precision 1 to that float oracle on the input sets of
tests/minsum_f32_sets.py.  The rest of this file shows that those sets can
tell: on every one the float oracle differs from the double oracle, and from
two float references mutated the way a kernel could plausibly be wrong (the
column sum taken in double and rounded once; taken from the last check to the
first) -- except that on a code whose columns have at most two checks both
mutations are the same arithmetic as the reference's (0 + a + b rounds once
and commutes), which is asserted too.  profiles/round18/minsum_f32_parity.txt
records the counts."""
import numpy as np
import pytest

import minsum_f32_sets as ms
import minsum_ref as mr
import shape_cases as sc
from oracle import oracle as orc

KEYS = mr.KEYS
BIG_FRAMES = 1      # frames of a large code's set that the numpy restatement decodes


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(out, ref, what):
    sc.eq(out, ref, what=what)
    sc.same_bits(out["post"], ref["post"], what=what)


# ---- inputs that pin the restatement ----------------------------------------------------

def pin_inputs():
    """(id, H, frames, cap): the reference's H at 0 / 2 / 4 dB, caps 5 and 50,
    two more of its matrices, and a large-code shape case."""
    out = []
    for db in (0, 2, 4):
        for cap in (5, 50):
            out.append(("default-db%d-cap%d" % (db, cap), "default", "db%d_llr" % db, cap))
    out += [("hData2", "other", "hData2", 20), ("hData5", "other", "hData5", 20),
            ("q_60x150", "case", "q_60x150", sc.CAP)]
    return out


def load(kind, key):
    if kind == "default":
        fd = ms.golden("frames_default.npz")
        return fd["H_reordered"], fd[key]
    if kind == "other":
        fo = ms.golden("frames_other.npz")
        return fo[key + "_H_reordered"], fo[key + "_llr"]
    c = sc.CASES[key]
    return np.array(c.H), c.frames


PIN = pin_inputs()


@pytest.mark.parametrize("kind,key,cap", [p[1:] for p in PIN], ids=[p[0] for p in PIN])
def test_float64_restatement_equals_the_oracle(kind, key, cap):
    H, y = load(kind, key)
    M, N = H.shape
    rp, ci = orc.dense_to_csr(H)
    ref = orc.decode_batch(0, H, y, cap, nthreads=sc.threads(), want_post=True)
    if kind == "case":
        sp = orc.decode_batch_sparse(0, rp, ci, M, N, y, cap, nthreads=sc.threads())
        sc.eq(sp, ref, what="sparse vs dense oracle")
    out = mr.decode((M, N, rp, ci), y, cap, Real=np.float64)
    same(out, ref, "%s cap %d, float64" % (key, cap))
    if kind == "default":      # and the fixtures the oracle wrote
        fd = ms.golden("frames_default.npz")
        pre = "%s_m0_i%d_" % (key[:3], cap)
        same(out, {k: fd[pre + k] for k in KEYS + ("post",)}, "fixture " + pre)


@pytest.mark.parametrize("et,polarity", [(1, 1.0), (5, 1.0), (1, -1.0), (5, -1.0)])
@pytest.mark.parametrize("kind,key,cap", [p[1:] for p in PIN], ids=[p[0] for p in PIN])
def test_float32_restatement_equals_the_float_oracle(kind, key, cap, et, polarity):
    H, y = load(kind, key)
    M, N = H.shape
    rp, ci = orc.dense_to_csr(H)
    ref = orc.decode_batch(0, H, y, cap, nthreads=sc.threads(), want_post=True, et_period=et,
                           polarity=polarity, real="f32")
    out = mr.decode((M, N, rp, ci), y, cap, Real=np.float32, et_period=et, polarity=polarity)
    same(out, ref, "%s cap %d et %d polarity %g, float32" % (key, cap, et, polarity))
    # the same options at float64, against the double oracle
    ref = orc.decode_batch(0, H, y, cap, nthreads=sc.threads(), want_post=True, et_period=et,
                           polarity=polarity)
    out = mr.decode((M, N, rp, ci), y, cap, Real=np.float64, et_period=et, polarity=polarity)
    same(out, ref, "%s cap %d et %d polarity %g, float64" % (key, cap, et, polarity))


EDGE_SETS = ["edge/" + k for k in ms.EDGES] + ["edge/degree_one_row"] + [
    "special/" + n for n in ms.SPECIAL]


@pytest.mark.parametrize("et", [1, 5])
@pytest.mark.parametrize("name", EDGE_SETS)
def test_float32_restatement_on_special_samples(name, et):
    s = ms.get(name)
    M, N, rp, ci = s.csr
    for real, Real in (("f32", np.float32), ("f64", np.float64)):
        ref = orc.decode_batch(0, s.H, s.y, s.cap, nthreads=sc.threads(), want_post=True,
                               et_period=et, real=real)
        out = mr.decode(s.csr, s.y, s.cap, Real=Real, et_period=et)
        same(out, ref, "%s et %d %s" % (name, et, real))


# ---- the oracle's interface -----------------------------------------------------------------

def test_float_oracle_dense_and_sparse_forms_and_strides():
    fd = ms.golden("frames_default.npz")
    H, y = fd["H_reordered"], fd["db2_llr"]
    M, N = H.shape
    rp, ci = orc.dense_to_csr(H)
    a = orc.decode_batch(0, H, y, 50, want_post=True, real="f32")
    b = orc.decode_batch_sparse(0, rp, ci, M, N, y, 50, want_post=True, real="f32", nthreads=4)
    same(a, b, "dense vs sparse form, 1 vs 4 threads")
    assert "post" not in orc.decode_batch(0, H, y, 50, real="f32")
    # interleaved complex samples at a one-sample stride, negated
    z = np.zeros(2 * y[:40].size + 10, np.float32)
    z[10::2] = y[:40].reshape(-1)
    z[11::2] = 7.0
    got = orc.decode_batch(0, H, z[10:], 50, polarity=-1.0, cw_stride=2, elem_stride=2, B=30,
                           want_post=True, real="f32")
    fr = np.stack([z[10 + 2 * b:10 + 2 * b + 2 * N:2] for b in range(30)])
    same(got, orc.decode_batch(0, H, -fr, 50, want_post=True, real="f32"), "strided, negated")


@pytest.mark.parametrize("method", [1, 2, 3])
def test_float_oracle_is_min_sum_only(method):
    fd = ms.golden("frames_default.npz")
    H, y = fd["H_reordered"], fd["db2_llr"]
    M, N = H.shape
    rp, ci = orc.dense_to_csr(H)
    with pytest.raises(ValueError, match="min-sum"):
        orc.decode_batch(method, H, y, 5, real="f32")
    with pytest.raises(ValueError, match="min-sum"):
        orc.decode_batch_sparse(method, rp, ci, M, N, y, 5, real="f32")
    with pytest.raises(ValueError, match="real"):
        orc.decode_batch(0, H, y, 5, real="f16")


# ---- every input set of the GPU tests can tell ------------------------------------------------

def small_enough(s):
    """The set itself, or the first frames of a large code's (the numpy
    restatement is the only double reference that returns its posteriors)."""
    return s if s.H is not None else s.head(BIG_FRAMES)


def differing(a, b):
    """Frames whose posterior bit patterns / hard decisions / iterations differ."""
    return (int((bits_of(a["post"]) != bits_of(b["post"])).any(axis=1).sum()),
            int((a["bits"] != b["bits"]).any(axis=1).sum()), int((a["iters"] != b["iters"]).sum()))


def double_reference(s):
    if s.H is not None:
        return s.ref64()
    return mr.decode(s.csr, s.y, s.cap, Real=np.float64, et_period=s.et, polarity=s.polarity)


@pytest.mark.parametrize("name", list(ms.SETS))
def test_every_set_separates_float_from_double(name):
    s = small_enough(ms.get(name))
    f32, f64 = s.ref(), double_reference(s)
    post, bits, iters = differing(f32, f64)
    print("%s: %d frames; float vs double differ in posterior bits %d, decisions %d, "
          "iterations %d" % (name, s.y.shape[0], post, bits, iters))
    assert post >= 1, name
    if name.startswith("default/"):
        assert post == s.y.shape[0], name
    if name == "default/db0/cap50":
        assert bits >= 1
    if name == "edge/overflow":
        # the double posteriors before the cast to float, from the restatement
        wide = mr.decode(s.csr, s.y, s.cap, Real=np.float64)["post_real"]
        lost = ~np.isfinite(f32["post"]) & np.isfinite(wide)
        print("%s: float posteriors inf %d, NaN %d, of them finite in double %d (in %d frames)" % (
            name, np.isinf(f32["post"]).sum(), np.isnan(f32["post"]).sum(), lost.sum(),
            lost.any(axis=1).sum()))
        assert lost.any(axis=1).sum() >= 1


@pytest.mark.parametrize("name", list(ms.SETS))
def test_every_set_separates_the_mutated_references(name):
    s = small_enough(ms.get(name))
    f32 = s.ref()
    kw = dict(et_period=s.et, polarity=s.polarity)
    for what, mut in (("column sum in double", dict(accumulate=np.float64)),
                      ("descending row order", dict(descending=True))):
        out = mr.decode(s.csr, s.y, s.cap, Real=np.float32, **mut, **kw)
        post, bits, iters = differing(out, f32)
        print("%s, %s: differs from the float reference in posterior bits %d, decisions %d, "
              "iterations %d of %d frames" % (name, what, post, bits, iters, s.y.shape[0]))
        if s.dv_max <= 2:
            # 0 + a + b: one rounding, and a + b == b + a -- not a different function
            assert (post, bits, iters) == (0, 0, 0), (name, what)
        else:
            assert post >= 1, (name, what)
