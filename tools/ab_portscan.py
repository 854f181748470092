#!/usr/bin/env python3
"""Cost of the port-scan detector (ppe_portscan_*) on the C1 workload (diagnostics): 1M x 64-B packets, 256 rules,
packed results, through one engine with the table attached and detached in alternation, the same build.

Two batches: `distinct` (every packet its own source address: the reference's 100,000-record pool fills, the rest is
NOMEM) and `hitter` (the same batch with one source owning 25 % of it, a new destination port per packet).  Each round
ages the table empty, moves the clock, and times --calls ppe_classify calls with events on one stream; microseconds per
call = per 1M packets.  The pre-pass's per-kernel split comes from a kernel trace of this tool (--calls 2 --rounds 1).

  python tools/ab_portscan.py [--calls 10] [--rounds 5] [--capacity 0]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppe import Engine, synth  # noqa: E402

NOW = 1_700_000_000


def batches(n, rules):
    pk = synth.make_packets(n, rules, kind="udp64", stride=64, malformed_frac=0.0)
    hdr = pk["hdr"].copy()
    sip = (0x0B000000 + np.arange(n)).astype(np.uint32)
    for k in range(4):
        hdr[:, 26 + k] = (sip >> (24 - 8 * k)) & 0xFF
    hit = hdr.copy()
    own = np.flatnonzero(np.random.default_rng(1).random(n) < 0.25)
    hit[own, 26:30] = (10, 9, 8, 7)
    port = (1 + np.arange(len(own)) % 60000).astype(np.uint32)
    hit[own, 36], hit[own, 37] = port >> 8, port & 0xFF
    return {"distinct": hdr, "hitter": hit}, pk["len"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=0, help="record pool (0: the reference's 100,000)")
    ap.add_argument("--packets", type=int, default=1 << 20)
    a = ap.parse_args()
    n = a.packets
    rules = synth.make_rules(synth.CONFIGS["C1"]["rules"])
    hdrs, lens = batches(n, rules)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    eng = Engine(0)
    eng.commit(rules, default_action=1)
    ps = eng.portscan(attach=False, capacity=a.capacity, max_batch=n)
    tl = torch.from_numpy(lens.view(np.int32)).to(dev)
    out = {"packed": torch.empty(n, dtype=torch.int64, device=dev), "part8": torch.empty(n, dtype=torch.uint8, device=dev)}
    cfg = eng.cfg(now_seconds=NOW)
    rate = 10**9
    for name, hdr in hdrs.items():
        th = torch.from_numpy(hdr).to(dev)
        us = {"detached": [], "attached": []}
        for r in range(a.rounds + 1):  # round 0: warm-up
            for mode in ("detached", "attached"):
                if mode == "attached":
                    ps.age((r + 2) * 100 * rate)          # empty table, the same start every round
                    ps.clock((r + 2) * 100 * rate + 1, NOW + r)
                    ps.attach()
                else:
                    ps.detach()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(stream)
                for _ in range(a.calls):
                    eng.classify_torch(th, tl, out, cfg=cfg, stream=stream)
                e1.record(stream)
                torch.cuda.synchronize()
                if r:
                    us[mode].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        ps.detach()
        info = ps.info()
        d, t = statistics.median(us["detached"]), statistics.median(us["attached"])
        print(f"{name:>9}: detached {d:8.1f} us / 1M packets (min {min(us['detached']):.1f}, max {max(us['detached']):.1f})  "
              f"attached {t:8.1f} (min {min(us['attached']):.1f}, max {max(us['attached']):.1f})  "
              f"detector {t - d:8.1f} us  [live {info['live']}, ok {info['ok']}, nomem {info['nomem']}, "
              f"detected {info['detected']}, hold {info['hold']}]", flush=True)
    ps.close()
    eng.close()


if __name__ == "__main__":
    main()
