"""bench.py's plain run and `--dump-outputs`: a plain run prints the headline line only (no nested configs, no
baselines: those are `--full`), `--steps` is the number of timed steps, and the dumped arrays are the last timed
step's outputs: float32 / float64 files, exact, equal to the oracle's answers for that step's (seeded) batch."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench
import pyoracle
from ppe import synth

ROOT = Path(__file__).resolve().parent.parent


def test_dump_outputs_exact_and_within_budget(tmp_path):
    small = {"w": np.array([0, 1, 0xFFFFFFFF], np.uint32), "h": np.array([-1, 7, 255], np.int32),
             "b": np.array([0, 191, 255], np.uint8), "one": np.uint32(5)}
    bench.dump_outputs(tmp_path / "s", small)
    got = {k: np.load(tmp_path / "s" / f"{k}.npy") for k in small}
    assert got["w"].dtype == got["h"].dtype == np.float64 and got["b"].dtype == np.float32
    for k, a in small.items():
        assert np.array_equal(got[k], np.atleast_1d(a).astype(np.float64))
    # past the budget: the same seeded, sorted rows of every array, from run to run
    n = 5 << 20
    big = {"x": np.arange(n, dtype=np.uint32), "y": np.arange(n, dtype=np.int32)[::-1]}
    for d in ("b1", "b2"):
        bench.dump_outputs(tmp_path / d, big)
    files = list((tmp_path / "b1").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= bench.DUMP_BUDGET
    x, y = np.load(tmp_path / "b1" / "x.npy"), np.load(tmp_path / "b1" / "y.npy")
    assert len(x) == len(y) > n // 2 and (np.diff(x) > 0).all() and np.array_equal(y, n - 1 - x)
    assert np.array_equal(x, np.load(tmp_path / "b2" / "x.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    n, steps = 65536, 3
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--n", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["steps"] == steps and d["value"] > 0 and d["unit"] == "Mpps" and d["higher_is_better"] is True
    assert d["ms_per_step"] == pytest.approx(n / d["value"] / 1e3, rel=1e-2)
    for k in ("configs", "cpu_baseline", "host_inclusive_mpps", "parity_sample_ok"):
        assert k not in d
    assert "dispatch" not in d["roofline"] and "ceiling" not in d["roofline"]
    # the last timed step ran on resident buffer (steps - 1) % nbufs = 2: generated batch 0 of rank 0
    cfgd = synth.CONFIGS["C1"]
    rules = synth.make_rules(cfgd["rules"])
    pk = synth.make_packets(n, rules, seed=synth.SEED + 1, kind=cfgd["kind"], stride=64)
    o = pyoracle.Oracle(rules, default_action=1)
    ref = o.classify_batch(pk["hdr"], pk["len"], cfg=o.cfg(now_seconds=bench.NOW))
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("verdict", "flow_hash", "acl_hit", "part8")}
    assert all(got[k].dtype == np.float64 and got[k].shape == (n,) for k in ("verdict", "flow_hash", "acl_hit"))
    assert got["part8"].dtype == np.float32
    assert (ref["reach"] <= 64).all()
    for k in ("verdict", "flow_hash", "acl_hit"):
        assert np.array_equal(got[k], ref[k].astype(np.float64)), k
    # the compact partition list (include/ppe_hip.h ppe_result_t.part8): per 64-packet tile FW, PUNT, DROP, stable
    act = (ref["verdict"] >> 8) & 0xFF
    order = np.argsort((np.arange(n) // 64) * 4 + np.array([0, 2, 1], np.int64)[act], kind="stable")
    assert np.array_equal(got["part8"], ((order & 63) | (act[order] << 6)).astype(np.float32))
