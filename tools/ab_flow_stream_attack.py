#!/usr/bin/env python3
"""Cost of the attack monitors with TCP sessions on the flow-table path (diagnostics): flow batches of
1 .. MAX packets (header stride 144, a port byte per packet) through ppe_classify_flow on an engine with monitors
flow-attached, sessions attached and ppe_flow_stream_monitors on (kind 6), against two yardsticks in the same process
and build: a twin with sessions only (kind 5) and a twin with monitors only (kinds 0 / 1 launches as the plain path
takes them).  tools/ab_flow_stream.py's workloads (udp / est-data / handshakes / one-flow).  The monitors' rules are
all zero: they count and drop nothing.

Per workload and size: --rounds rounds of --calls calls enqueued back to back on one stream; stream us per call (events
around the calls), median (min-max) over the rounds; each yardstick runs twice per round, and the spread between its
two medians is the run's A/A spread.

Then ppe_flow_age on a table of 65,536 flows left in SYN_SENT, wall us per call, with the decrement pass (the switch
on) and without it (the switch off for the call).

  python tools/ab_flow_stream_attack.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "tools"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stream_session_corpus as sc  # noqa: E402
from ab_flow_stream import FW, STRIDE, fmt, syn, workloads  # noqa: E402
from ppe import Engine, abi  # noqa: E402


def engine(sessions, monitors, cap, max_batch):
    e = Engine(0)
    e.commit(np.zeros(0, abi.RULE_DTYPE), default_action=FW)
    e.flow_create(cap, max_batch)
    if sessions:
        e.stream_tcp(track=1, reasm=0)
        e.flow_stream(1)
    atk = e.attack(None, attach="flow") if monitors else None
    e.flow_stream_monitors(1 if sessions and monitors else 0)
    return e, atk


def classify_part(a):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    to = lambda h, ln: (torch.from_numpy(h).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev))  # noqa: E731
    print(f"ppe_classify_flow, stride {STRIDE}, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    for n in a.sizes:
        ports = torch.from_numpy(np.random.default_rng(n).integers(0, 4, max(n, 3)).astype(np.uint8)).to(dev)
        for name, (prime, batches, aged) in workloads(n, a.calls).items():
            engs = {"both": engine(True, True, 1 << 19, 2048), "sess": engine(True, False, 1 << 19, 2048),
                    "mon": engine(False, True, 1 << 19, 2048)}
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
            for e, atk in engs.values():
                if atk is not None:
                    atk.ports([ports])
                for h, ln in prime:
                    th, tl = to(h, ln)
                    po = {k: torch.empty(len(ln), dtype=torch.int32, device=dev) for k in out}
                    e.classify_flow_torch(th, tl, po, cfg=e.cfg(0, 1, 1001), stream=stream)
                    torch.cuda.synchronize()
            dv = [to(h, ln) for h, ln in batches]
            modes = ("sess", "mon", "both", "sess2", "mon2")
            gpu = {k: [] for k in modes}
            for r in range(a.rounds + 1):  # round 0: warm-up
                for mode in modes:
                    e, atk = engs[mode.rstrip("2")]
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
            aa = {k: abs(statistics.median(gpu[k]) - statistics.median(gpu[k + "2"])) for k in ("sess", "mon")}
            kinds = {k: engs[k][0].flow_launch_info() for k in engs}
            print(f"n {n:5d} {name:>10}: both {fmt(gpu['both'])}  sessions {fmt(gpu['sess'])}  again {fmt(gpu['sess2'])}  "
                  f"A/A {aa['sess']:.2f}  monitors {fmt(gpu['mon'])}  again {fmt(gpu['mon2'])}  A/A {aa['mon']:.2f}  "
                  f"[kind, launches: {kinds['both']} / {kinds['sess']} / {kinds['mon']}]", flush=True)
            for e, atk in engs.values():
                if atk is not None:
                    atk.close()
                e.flow_destroy()
                e.close()


def age_part(a):
    n = 65536
    hdr, lens = sc.batch([syn(f) for f in range(n)], STRIDE)
    ports = np.random.default_rng(1).integers(0, 4, n).astype(np.uint8)
    e, atk = engine(True, True, 1 << 17, 4096)
    us = {"with": [], "without": []}
    for r in range(a.rounds + 1):
        for k, mode in enumerate(us):
            now = 1000 + 100 * (2 * r + k)
            e.classify_flow_host_ports(hdr, lens, ports, cfg=e.cfg(0, 1, now), outputs=("verdict",))
            e.flow_stream_monitors(1 if mode == "with" else 0)
            w0 = time.perf_counter()
            d = e.flow_age(now + 50, 1)
            w1 = time.perf_counter()
            e.flow_stream_monitors(1)
            atk.tick(now + 50)
            assert d == n, d
            if r:
                us[mode].append((w1 - w0) * 1e6)
    print(f"ppe_flow_age, {n} flows in SYN_SENT deleted, wall us per call: with the decrement pass {fmt(us['with'])}  "
          f"without {fmt(us['without'])}", flush=True)
    atk.close()
    e.flow_destroy()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024])
    a = ap.parse_args()
    classify_part(a)
    age_part(a)


if __name__ == "__main__":
    main()
