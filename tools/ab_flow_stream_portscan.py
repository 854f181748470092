#!/usr/bin/env python3
"""Cost of the port-scan detector with TCP sessions on the flow-table path (diagnostics): flow batches
of 1 .. MAX packets (header stride 144, a port byte per packet) through ppe_classify_flow on an engine with a port-scan
table flow-attached, sessions attached and ppe_flow_stream_portscan on, without the monitors (kind 7) and with them
(kind 8), against four yardsticks in the same process and build: twins with the detector and no sessions (kinds 2 / 3)
and twins with sessions and no detector (kinds 5 / 6).  tools/ab_flow_stream.py's workloads (udp / est-data /
handshakes / one-flow) and one-scanner: n SYNs of one source to n ports, a new client port per call, so every call is
one source's chain of n resolve rounds and n new sessions.  The monitors' rules are all zero and the detector's clock
stands still: nothing is dropped.

Per workload and size: --rounds rounds of --calls calls enqueued back to back on one stream; stream us per call (events
around the calls), median (min-max) over the rounds; each yardstick runs twice per round, and the spread between its
two medians is the run's A/A spread.

  python tools/ab_flow_stream_portscan.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "tools"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_flow_stream import FW, STRIDE, fmt, workloads  # noqa: E402
from pktbuild import tcp_packet  # noqa: E402
from ppe import Engine, abi  # noqa: E402

# name -> (sessions, detector, monitors)
ENGINES = {"k7": (True, True, False), "k8": (True, True, True), "det": (False, True, False), "det_mon": (False, True, True),
           "sess": (True, False, False), "sess_mon": (True, False, True)}
YARD = ("det", "det_mon", "sess", "sess_mon")


def engine(sessions, detector, monitors, cap, max_batch):
    e = Engine(0)
    e.commit(np.zeros(0, abi.RULE_DTYPE), default_action=FW)
    e.flow_create(cap, max_batch)
    if sessions:
        e.stream_tcp(track=1, reasm=0)
        e.flow_stream(1)
    ps = e.portscan(attach="flow", able=1, max_batch=max_batch) if detector else None
    atk = e.attack(None, attach="flow") if monitors else None
    e.flow_combine(1 if detector and monitors else 0)
    e.flow_stream_monitors(1 if sessions and monitors else 0)
    e.flow_stream_portscan(1 if sessions and detector else 0)
    return e, ps, atk


def scanner(n, calls):
    """Per call one batch: n SYNs of one source to ports 1 .. n from client port 1024 + call."""
    out = []
    for c in range(calls):
        hdr = np.zeros((n, STRIDE), np.uint8)
        lens = np.zeros(n, np.uint32)
        for i in range(n):
            f = tcp_packet(0x0A000001, 0xAC100001, 1024 + c, 1 + i)
            hdr[i, :len(f)] = np.frombuffer(f, np.uint8)
            lens[i] = len(f)
        out.append((hdr, lens))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    to = lambda h, ln: (torch.from_numpy(h).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev))  # noqa: E731
    print(f"ppe_classify_flow, stride {STRIDE}, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    for n in a.sizes:
        ports = torch.from_numpy(np.random.default_rng(n).integers(0, 4, max(n, 3)).astype(np.uint8)).to(dev)
        loads = workloads(n, a.calls)
        loads["one-scanner"] = ([], scanner(n, a.calls), True)
        for name, (prime, batches, aged) in loads.items():
            engs = {k: engine(*v, 1 << 19, 2048) for k, v in ENGINES.items()}
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
            for e, ps, atk in engs.values():
                if atk is not None:
                    atk.ports([ports])
                for h, ln in prime:
                    th, tl = to(h, ln)
                    po = {k: torch.empty(len(ln), dtype=torch.int32, device=dev) for k in out}
                    e.classify_flow_torch(th, tl, po, cfg=e.cfg(0, 1, 1001), stream=stream)
                    torch.cuda.synchronize()
            dv = [to(h, ln) for h, ln in batches]
            modes = YARD + ("k7", "k8") + tuple(k + "2" for k in YARD)
            gpu = {k: [] for k in modes}
            for r in range(a.rounds + 1):  # round 0: warm-up
                for mode in modes:
                    e, ps, atk = engs[mode.rstrip("2")]
                    now = 1001
                    if aged and r:
                        now = 1001 + 100 * (len(modes) * r + modes.index(mode))
                        e.flow_age(now, 1)
                    if atk is not None:
                        atk.tick(now)
                    cfg = e.cfg(0, 1, now)
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
            aa = {k: abs(statistics.median(gpu[k]) - statistics.median(gpu[k + "2"])) for k in YARD}
            kinds = {k: engs[k][0].flow_launch_info() for k in engs}
            print(f"n {n:5d} {name:>11}: k7 {fmt(gpu['k7'])}  k8 {fmt(gpu['k8'])}  " +
                  "  ".join(f"{k} {fmt(gpu[k])} again {fmt(gpu[k + '2'])} A/A {aa[k]:.2f}" for k in YARD) +
                  f"  [kind, launches: " + " / ".join(f"{k} {kinds[k]}" for k in engs) + "]", flush=True)
            for e, ps, atk in engs.values():
                if atk is not None:
                    atk.close()
                if ps is not None:
                    ps.close()
                e.flow_destroy()
                e.close()


if __name__ == "__main__":
    main()
