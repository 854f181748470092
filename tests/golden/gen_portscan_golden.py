"""Writes tests/golden/portscan_v1.npz: one scripted multi-batch scenario of tests/portscan_model.py, frozen, so that
a change of the model shows (tests/test_portscan.py replays it; tests/test_gpu_portscan.py runs it on the GPU).

Run from the repository root: python tests/golden/gen_portscan_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "packet-process-engine_amd")]

from portscan_model import PortScanModel  # noqa: E402

CFG = dict(able=1, action=0, exception_freq=3, hold_seconds=5, capacity=6, cycles_per_second=1000)


def scenario():
    """Batches of (now_cycles, now_seconds, sip[], dport[], ts[]): eight sources against six records, a scanner that
    is detected, held and released, port 0, repeats, the 1-2 s roll, a reset, and an aging pass after batch 5."""
    rng = np.random.default_rng(20261020)
    out = []
    t0, s0 = 50_000, 1_700_000_000
    for b, dc in enumerate((0, 400, 1500, 1900, 2600, 9000, 9100, 40_000)):
        n = (5, 64, 130, 33, 200, 17, 96, 40)[b]
        sip = 0x0A000001 + rng.integers(0, 8, n).astype(np.uint32)
        dport = rng.choice(np.array([0, 22, 22, 80, 443, 8080, 53], np.uint32), n)
        scan = sip == 0x0A000003                        # the scanner: a new port nearly every packet
        dport[scan] = 1000 + np.arange(int(scan.sum()), dtype=np.uint32) // 2 * (b + 1)
        ts = np.uint64(s0 + dc // 1000) + rng.integers(0, 3, n).astype(np.uint64)
        out.append((t0 + dc, s0 + dc // 1000, sip, dport, ts))
    return out


def run():
    m = PortScanModel(**CFG)
    res, recs = {}, {}
    for b, (nc, ns, sip, dport, ts) in enumerate(scenario()):
        m.clock(nc, ns)
        res[f"res{b}"] = np.array(m.batch(sip, dport, ts), np.int8)
        for k, v in (("sip", sip), ("dport", dport), ("ts", ts)):
            res[f"{k}{b}"] = v
        res[f"clock{b}"] = np.array([nc, ns], np.uint64)
        if b == 5:
            res["freed5"] = np.array([m.timeout(nc + 25_000)], np.int64)
        recs[f"rec{b}"] = np.array(sorted(m.records()), np.uint64).reshape(-1, 7)
    info = m.info()
    res["info"] = np.array([info[k] for k in sorted(info)], np.int64)
    return {**res, **recs}


if __name__ == "__main__":
    np.savez_compressed(ROOT / "tests" / "golden" / "portscan_v1.npz", **run())
