#!/usr/bin/env python3
"""Cost of the attack monitors on the flow-table path (ppe_flow_attack_attach) on the F1 workload (diagnostics): 1M x
64-B packets over 2^18 flows through ppe_classify_flow, one engine with the object flow-attached and detached in
alternation, the same build, one process.  The sibling of tools/ab_attack.py (the stateless path).

Three settings: `zero` (all-zero rules, no port array), `ports` (the same with a port array: one more byte read per
packet, and per SYN-created flow in the post launch), `flood` (a UDP flood on every port dropping every UDP
packet before the flow table).  Each round times --calls ppe_classify_flow calls with events on one
stream, detached A, attached, detached B; microseconds per call = per 1M packets; detached A against detached B is the
noise floor.  A second pass per mode reads the classify launches' own dispatch times (ppe_timing_read), so the delta
splits into the classify launch and the rest of the call (the post launch and the gaps).

  python tools/ab_attack_flow.py [--calls 10] [--rounds 5]
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
    ap.add_argument("--packets", type=int, default=synth.CONFIGS["F1"]["n"])
    ap.add_argument("--flows", type=int, default=synth.CONFIGS["F1"]["flows"])
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--nbufs", type=int, default=8)
    a = ap.parse_args()
    n = a.packets
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    flood = abi.AttackCfg.make(td={p: dict(drop_pack=1, flood_udp=1, udp_speed=0) for p in range(4)})
    rules = synth.make_rules(synth.CONFIGS["F1"]["rules"])
    eng = Engine(0)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)   # (as bench.py's F1: every flow gets created)
    eng.flow_create(2 * a.flows, n)
    atk = eng.attack(attach=False)
    bufs = []
    tseed = synth.SEED + 977                  # (bench.py's F1 population and batches)
    for b in range(a.nbufs):
        pk = synth.make_flow_packets(n, rules, a.flows, seed=tseed + 7919 * (b + 1), template_seed=tseed, stride=64)
        bufs.append((torch.from_numpy(pk["hdr"]).to(dev), torch.from_numpy(pk["len"].view(np.int32)).to(dev)))
    tp = torch.from_numpy((np.arange(n) % 4).astype(np.uint8)).to(dev)
    out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
    out["part8"] = torch.empty(n, dtype=torch.uint8, device=dev)
    step = [0]

    def calls(k):
        for _ in range(k):
            th, tl = bufs[step[0] % a.nbufs]
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(now_seconds=NOW + step[0]), stream=stream)
            step[0] += 1

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        calls(a.calls)
        e1.record(stream)
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) * 1e3 / a.calls
        eng.timing(True)                      # the classify launches' own dispatch times, in a pass of their own
        eng.timing_read(reset=True)
        calls(a.calls)
        torch.cuda.synchronize()
        ms, launches = eng.timing_read(reset=True)
        eng.timing(False)
        return total, ms * 1e3 / max(launches, 1)

    import time
    t0 = time.time()                          # the table warm (every flow exists) and the clocks ramped, as bench.py does
    while time.time() - t0 < a.warm_seconds:
        calls(8)
        torch.cuda.synchronize()
    for setting in ("zero", "ports", "flood"):
        atk.set(flood if setting == "flood" else abi.AttackCfg.make())
        atk.ports([tp] if setting != "zero" else None)
        us = {"detached_a": [], "attached": [], "detached_b": []}
        for r in range(a.rounds + 1):  # round 0: warm-up
            for mode in us:
                if mode == "attached":
                    atk.attach_flow()
                    atk.tick(NOW + r)          # pps = the previous round's count: the flood setting drops
                else:
                    atk.detach_flow()
                t = timed()
                if r:
                    us[mode].append(t)
        atk.detach_flow()
        med = {k: (statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)) for k, v in us.items()}
        base, base_k = [(med["detached_a"][i] + med["detached_b"][i]) / 2 for i in (0, 1)]
        det = [x[0] for x in us["detached_a"] + us["detached_b"]]
        att = [x[0] for x in us["attached"]]
        info = atk.info()
        d, dk = med["attached"][0] - base, med["attached"][1] - base_k
        print(f"F1 {setting:>5}: detached {med['detached_a'][0]:7.2f} / {med['detached_b'][0]:7.2f} us per call "
              f"(A/A {med['detached_b'][0] - med['detached_a'][0]:+.2f}; min {min(det):.2f}, max {max(det):.2f})  "
              f"attached {med['attached'][0]:7.2f} (min {min(att):.2f}, max {max(att):.2f})  monitors {d:+.2f} us = "
              f"{100 * d / base:+.1f} %  |  classify launch {base_k:.2f} -> {med['attached'][1]:.2f} ({dk:+.2f}), "
              f"rest of the call {d - dk:+.2f}  [udpflood_drop {info['udpflood_drop']}]", flush=True)
    atk.close()
    eng.flow_destroy()
    eng.close()


if __name__ == "__main__":
    main()
