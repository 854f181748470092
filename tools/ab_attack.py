#!/usr/bin/env python3
"""Cost of the attack monitors (ppe_attack_*) on the C1 and C4 workloads (diagnostics): 1M x 64-B packets, packed
results, through one engine with the object attached and detached in alternation, the same build, one process.

Three settings: `zero` (all-zero rules, no port array: the decision word, the accumulator counts and their flush),
`ports` (the same with a port array: one more byte read per packet), `flood` (a UDP flood on every port dropping every
UDP packet).  Each round times --calls ppe_classify calls with events on one stream, detached A, attached, detached B;
microseconds per call = per 1M packets.  The yardstick is the detached context of the same library in the same
process; detached A against detached B is the noise floor.

  python tools/ab_attack.py [--calls 10] [--rounds 5] [--configs C1,C4]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppe import Engine, abi, synth  # noqa: E402

NOW = 1_700_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="C1,C4")
    ap.add_argument("--packets", type=int, default=1 << 20)
    a = ap.parse_args()
    n = a.packets
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    flood = abi.AttackCfg.make(td={p: dict(drop_pack=1, flood_udp=1, udp_speed=0) for p in range(4)})
    for name in a.configs.split(","):
        rules = synth.make_rules(synth.CONFIGS[name]["rules"])
        pk = synth.make_packets(n, rules, kind="udp64", stride=64, malformed_frac=0.0)
        eng = Engine(0)
        eng.commit(rules, default_action=1)
        atk = eng.attack(attach=False)
        th = torch.from_numpy(pk["hdr"]).to(dev)
        tl = torch.from_numpy(pk["len"].view(np.int32)).to(dev)
        tp = torch.from_numpy((np.arange(n) % 4).astype(np.uint8)).to(dev)
        out = {"packed": torch.empty(n, dtype=torch.int64, device=dev),
               "part8": torch.empty(n, dtype=torch.uint8, device=dev)}
        cfg = eng.cfg(now_seconds=NOW)

        def timed():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(a.calls):
                eng.classify_torch(th, tl, out, cfg=cfg, stream=stream)
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.calls

        for setting in ("zero", "ports", "flood"):
            atk.set(flood if setting == "flood" else abi.AttackCfg.make())
            atk.ports([tp] if setting != "zero" else None)
            us = {"detached_a": [], "attached": [], "detached_b": []}
            for r in range(a.rounds + 1):  # round 0: warm-up
                for mode in us:
                    if mode == "attached":
                        atk.attach()
                        atk.tick(NOW + r)      # pps = the previous round's count: the flood setting drops
                    else:
                        atk.detach()
                    t = timed()
                    if r:
                        us[mode].append(t)
            atk.detach()
            med = {k: statistics.median(v) for k, v in us.items()}
            base = (med["detached_a"] + med["detached_b"]) / 2
            info = atk.info()
            print(f"{name} {setting:>5}: detached {med['detached_a']:7.2f} / {med['detached_b']:7.2f} us per 1M packets "
                  f"(A/A {med['detached_b'] - med['detached_a']:+.2f}; min {min(us['detached_a'] + us['detached_b']):.2f}, "
                  f"max {max(us['detached_a'] + us['detached_b']):.2f})  attached {med['attached']:7.2f} "
                  f"(min {min(us['attached']):.2f}, max {max(us['attached']):.2f})  monitors {med['attached'] - base:+.2f} us "
                  f"= {100 * (med['attached'] - base) / base:+.1f} %  [udpflood_drop {info['udpflood_drop']}]", flush=True)
        atk.close()
        eng.close()


if __name__ == "__main__":
    main()
