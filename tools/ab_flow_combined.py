#!/usr/bin/env python3
"""Cost of the attack monitors inside the flow kernel with the port-scan detector (diagnostics): flow
batches of 1 .. MAX 64-B packets through ppe_classify_flow on an engine with a port-scan table and an attack object both
flow-attached and ppe_flow_combine on (the combined kernel, ppe_flow_launch_info kind 3) and on a twin with only the
table flow-attached (the kernel with the detector alone, kind 2: the yardstick), the modes alternating in one process,
the same build.  The monitors' rules are all zero and every packet is on a port of a four-port array: the monitors
count and drop nothing, so both kernels decide the same packets the same way.  Workloads:
  found      a warm table, every packet finds its flow
  newflows   every packet a TCP SYN of a new flow from a source of its own (a different batch per call; the table is
             aged empty between the rounds): every packet a creator counted in syncount_accum
  mixed      tests/flow_portscan_model.py's generated batch (8 sources, 6 ports, both directions)

Per workload and size: --rounds rounds of --calls calls enqueued back to back on one stream; stream us per call (events
around the calls), median (min-max) over the rounds; the twin runs twice per round, and the spread between its two
medians is the run's A/A spread.

  python tools/ab_flow_combined.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT / "tests"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flow_portscan_model as fpm  # noqa: E402
from pktbuild import tcp_packet, udp_packet  # noqa: E402
from ppe import Engine, abi  # noqa: E402

RATE = 1000
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f}-{max(v):.2f})"


def stack(frames):
    hdr = np.zeros((len(frames), 64), np.uint8)
    for i, f in enumerate(frames):
        hdr[i, :len(f)] = np.frombuffer(f, np.uint8)
    return hdr, np.array([len(f) for f in frames], np.uint32)


def any_rule():
    r = np.zeros(1, abi.RULE_DTYPE)
    r["sport_end"] = r["dport_end"] = 65535
    r["protocol_end"] = 255
    r["action"] = FW
    return r


def workloads(n, calls):
    """name -> (rules, default action, flow capacity, batches cycled over the calls, aged)."""
    srv = 0x0B000001
    udp = lambda k: udp_packet(0x0A000000 + k, srv, 1024 + (k & 0x7FFF), 53)  # noqa: E731
    syn = lambda k: tcp_packet(0x0A000000 + k, srv, 1024 + (k & 0x7FFF), 80, flags=0x02)  # noqa: E731
    return {
        "found": (any_rule(), DROP, 1 << 16, [stack([udp(k) for k in range(n)])], False),
        "newflows": (any_rule(), DROP, 1 << 19, [stack([syn(c * n + k) for k in range(n)]) for c in range(calls)], True),
        "mixed": (fpm.gen_rules(), DROP, 1 << 16, [fpm.gen_batch(np.random.default_rng(3), n)], False),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    print(f"ppe_classify_flow, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    for n in a.sizes:
        for name, (rules, dflt, cap, batches, aged) in workloads(n, a.calls).items():
            engs, pss = {}, {}
            for mode in ("combined", "table"):
                e = engs[mode] = Engine(0)
                e.commit(rules, default_action=dflt)
                e.flow_create(cap, 2048)
                pss[mode] = e.portscan(attach="flow", able=1, exception_freq=3, hold_seconds=600, capacity=1 << 19,
                                       max_batch=2048, cycles_per_second=RATE)
                pss[mode].clock(10 * RATE, 1000)
            atk = engs["combined"].attack(attach="flow")
            atk.clock(1000)
            ports = torch.from_numpy((np.arange(n) % 4).astype(np.uint8)).to(dev)
            atk.ports([ports])
            engs["combined"].flow_combine(1)
            dv = [(torch.from_numpy(h).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev)) for h, ln in batches]
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
            modes = ("table", "combined", "table2")
            gpu = {m: [] for m in modes}
            for r in range(a.rounds + 1):  # round 0: warm-up (and the batch's flows enter both tables)
                for mode in modes:
                    e = engs["combined" if mode == "combined" else "table"]
                    cfg = e.cfg(0, 1, 1001)
                    if aged and r:
                        e.flow_age(1001 + 100 * (3 * r + modes.index(mode)), 1)
                        cfg = e.cfg(0, 1, 1001 + 100 * (3 * r + modes.index(mode)))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(stream)
                    for c in range(a.calls):
                        th, tl = dv[c % len(dv)]
                        e.classify_flow_torch(th, tl, out, cfg=cfg, stream=stream)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if r:
                        gpu[mode].append(e0.elapsed_time(e1) * 1e3 / a.calls)
                    if mode == "combined":
                        atk.tick(1001 + r)
            aa = abs(statistics.median(gpu["table"]) - statistics.median(gpu["table2"]))
            kinds = {m: engs[m].flow_launch_info() for m in engs}
            info = atk.info()
            acc = [sum(p[k] for p in info["ai"]) for k in ("udppps", "synpps", "syncount")]
            print(f"n {n:5d} {name:>9}: combined {fmt(gpu['combined'])}  table only {fmt(gpu['table'])}  "
                  f"table only again {fmt(gpu['table2'])}  A/A spread {aa:.2f}  "
                  f"[kind, launches: {kinds['combined']} / {kinds['table']}; last interval udp/syn/syncount "
                  f"{acc[0]}/{acc[1]}/{acc[2]}]", flush=True)
            atk.close()
            for m in engs:
                pss[m].close()
                engs[m].flow_destroy()
                engs[m].close()


if __name__ == "__main__":
    main()
