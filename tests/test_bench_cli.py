"""bench.py's command line: what a plain run holds, what --full adds, and
--dump-outputs.

CPU: the option parsing and the dump writer (float32 files, the seeded frame
sample above the size limit).  GPU: one plain run as a child process with
--dump-outputs; the files must be the decode of the last timed step's batch
-- made again here from its seed -- as the oracle computes it, which also
shows that the inputs are the same from run to run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_plain_is_default_and_sweeps_need_full():
    a = bench.parse([])
    assert not a.full and a.dump_outputs is None
    assert bench.parse(["--full", "--sweep-batch", "64"]).full
    for opt in ("--sweep-batch", "--sweep-inflight", "--sweep-config5"):
        with pytest.raises(SystemExit):
            bench.parse([opt, "64"])


def _fake_outs(B, KB):
    rng = np.random.Generator(np.random.PCG64(9))
    return [("packed", torch.from_numpy(rng.integers(0, 256, size=(B, KB), dtype=np.uint8))),
            ("iters", torch.from_numpy(rng.integers(1, 51, size=B).astype(np.int32))),
            ("synd", torch.from_numpy(rng.integers(0, 33, size=B).astype(np.int32)))]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole(tmp_path):
    outs = _fake_outs(1187, 4)
    bench.dump_outputs(str(tmp_path / "d"), outs, 2024)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == ["iters", "packed", "synd"]
    for name, t in outs:
        assert got[name].dtype == np.float32
        assert got[name].shape == tuple(t.shape)
        assert (got[name] == t.numpy()).all()


def test_dump_outputs_sampled_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    outs = _fake_outs(4099, 4)  # 4099 * 24 bytes as float32: above the limit
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, 2024)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    size = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= 1 << 16
    keep = a["frame_index"]
    assert keep.dtype == np.float64 and (np.diff(keep) > 0).all()
    assert 1500 < keep.size < 4099 and keep.min() >= 0 and keep.max() < 4099
    idx = keep.astype(np.int64)
    for name, t in outs:
        assert a[name].dtype == np.float32
        assert (a[name] == t.numpy()[idx]).all()
        assert (a[name] == b[name]).all()  # the same sample every time
    assert (keep == b["frame_index"]).all()


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_step(tmp_path):
    import ldpc_ece535a as L
    from oracle import oracle as orc

    B, steps, warmup, seed = 300, 3, 2, 2024
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--batch", str(B), "--preroll-ms",
                        "1", "--dump-outputs", out], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["unit"] == "Mbit/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    # ms_per_step is the wall time of one timed step: value = info bits of a step / that
    # (the line rounds ms_per_step to 4 places and value to 3)
    ms = line["ms_per_step"]
    assert ms > 0
    assert line["value"] == pytest.approx(B * 32 / (ms * 1e-3) / 1e6, rel=5e-5 / ms + 1e-3)
    # a plain run measures the headline alone
    for k in ("cpu_baseline", "parity", "variants_1gpu", "serial_1_batch_in_flight"):
        assert k not in line
    got = _load(out)
    assert sorted(got) == ["iters", "packed", "synd"]
    # the last timed step posts batch (warmup + steps - 1) % D, made from its own seed
    dec = L.Decoder(device=0)
    j = (warmup + steps - 1) % 4
    y = bench.synth_device(L, torch, dec, B, 2.0, seed + 104729 * j, torch.device("cuda", 0))[0]
    ref = orc.decode_batch(1, dec.H, y.cpu().numpy(), 50, nthreads=4)
    dec.close()
    for name in ("packed", "iters", "synd"):
        assert got[name].dtype == np.float32
        assert (got[name] == ref[name]).all(), name
