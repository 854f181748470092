#!/usr/bin/env python3
"""Cost of the TCP session machine on the flow-table path (diagnostics): flow batches of 1 .. MAX
packets (header stride 144) through ppe_classify_flow on an engine with sessions attached and tracking on (the
one-launch kernel with the session phase) and on a twin with the switch off (today's kernels: the yardstick), the
modes alternating in one process, the same build.  Workloads:
  udp        a warm table, every packet UDP and found: the session phase has nothing to do
  est-data   n established connections, one data packet of each per batch
  handshakes whole handshakes (SYN, SYN|ACK, ACK) of new flows in one batch, other flows with every call; the table is
             aged empty between the rounds
  one-flow   one established flow owns the batch: n one-byte segments to the server, the longest walk

Per workload and size: --rounds rounds of --calls calls enqueued back to back on one stream; stream us per call (events
around the calls), median (min-max) over the rounds; the detached twin runs twice per round, and the spread between its
two medians is the run's A/A spread.

Then a 65,536-packet pageable ppe_classify_flow_host call (16,384 connections: handshake and one data packet), wall ns
per packet, attached against detached.

  python tools/ab_flow_stream.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT / "tests"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stream_session_corpus as sc  # noqa: E402
import stream_session_model as m  # noqa: E402
from pktbuild import udp_packet  # noqa: E402
from ppe import Engine, abi  # noqa: E402
from stream_session_corpus import A, P, S  # noqa: E402

STRIDE = 144
FW = abi.ACL_RULE_ACTION_FW


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f}-{max(v):.2f})"


def syn(f):
    return (f, m.Pkt(False, S, 1000, 0, 1000))


def synack(f):
    return (f, m.Pkt(True, S | A, 5000, 1001, 2000))


def ack(f):
    return (f, m.Pkt(False, A, 1001, 5001, 1000))


def data(f, k=0):
    return (f, m.Pkt(False, A | P, 1001 + k, 5001, 1000, 1))


def udp_batch(n):
    hdr = np.zeros((n, STRIDE), np.uint8)
    lens = np.zeros(n, np.uint32)
    for i in range(n):
        fr = udp_packet(0x0A000000 + i, 0x0B000001, 1024 + (i & 0x7FFF), 53)
        hdr[i, :len(fr)] = np.frombuffer(fr, np.uint8)
        lens[i] = len(fr)
    return hdr, lens


def workloads(n, calls):
    """name -> (prime batches run once on both engines, batches cycled over the calls, aged between the rounds)."""
    b = lambda seq: sc.batch(seq, STRIDE)  # noqa: E731
    flows = max(1, n // 3)
    hs = [b([p for f in range(c * flows, (c + 1) * flows) for p in (syn(f), synack(f), ack(f))][:n] if n >= 3
            else [syn(c)][:n]) for c in range(calls)]
    return {
        "udp": ([], [udp_batch(n)], False),
        "est-data": ([b([syn(f) for f in range(n)]), b([synack(f) for f in range(n)]), b([ack(f) for f in range(n)])],
                     [b([data(f) for f in range(n)])], False),
        "handshakes": ([], hs, True),
        "one-flow": ([b([syn(7), synack(7), ack(7)])], [b([data(7, k) for k in range(n)])], False),
    }


def engine(attached, cap, max_batch):
    e = Engine(0)
    e.commit(np.zeros(0, abi.RULE_DTYPE), default_action=FW)
    e.flow_create(cap, max_batch)
    if attached:
        e.stream_tcp(track=1, reasm=0)
        e.flow_stream(1)
    return e


def classify_part(a):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    to = lambda h, ln: (torch.from_numpy(h).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev))  # noqa: E731
    print(f"ppe_classify_flow, stride {STRIDE}, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    for n in a.sizes:
        for name, (prime, batches, aged) in workloads(n, a.calls).items():
            engs = {"attached": engine(True, 1 << 19, 2048), "detached": engine(False, 1 << 19, 2048)}
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
            for e in engs.values():
                for h, ln in prime:
                    th, tl = to(h, ln)
                    po = {k: torch.empty(len(ln), dtype=torch.int32, device=dev) for k in out}
                    e.classify_flow_torch(th, tl, po, cfg=e.cfg(0, 1, 1001), stream=stream)
                    torch.cuda.synchronize()
            dv = [to(h, ln) for h, ln in batches]
            modes = ("detached", "attached", "detached2")
            gpu = {k: [] for k in modes}
            for r in range(a.rounds + 1):  # round 0: warm-up
                for mode in modes:
                    e = engs["attached" if mode == "attached" else "detached"]
                    now = 1001
                    if aged and r:
                        now = 1001 + 100 * (3 * r + modes.index(mode))
                        e.flow_age(now, 1)
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
            aa = abs(statistics.median(gpu["detached"]) - statistics.median(gpu["detached2"]))
            kinds = {k: engs[k].flow_launch_info() for k in engs}
            drops = int(((out["verdict"].cpu().numpy().view(np.uint32) >> 8) & 0xFF == 1).sum())
            print(f"n {n:5d} {name:>10}: attached {fmt(gpu['attached'])}  detached {fmt(gpu['detached'])}  "
                  f"detached again {fmt(gpu['detached2'])}  A/A spread {aa:.2f}  "
                  f"[kind, launches: {kinds['attached']} / {kinds['detached']}; drops in the last batch {drops}]", flush=True)
            for e in engs.values():
                e.flow_destroy()
                e.close()


def host_part(a):
    n = 65536
    hdr, lens = sc.batch([p for f in range(n // 4) for p in (syn(f), synack(f), ack(f), data(f))], STRIDE)
    engs = {"attached": engine(True, 1 << 16, 4096), "detached": engine(False, 1 << 16, 4096)}
    modes = ("detached", "attached", "detached2")
    ns = {k: [] for k in modes}
    for r in range(a.rounds + 1):
        for k, mode in enumerate(modes):
            e = engs["attached" if mode == "attached" else "detached"]
            now = 1000 + 100 * (3 * r + k)
            e.flow_age(now, 1)  # (an empty table every time: the batch creates its 16,384 flows)
            w0 = time.perf_counter()
            e.classify_flow_host(hdr, lens, cfg=e.cfg(0, 1, now), outputs=("verdict", "flow_hash", "acl_hit"))
            w1 = time.perf_counter()
            if r:
                ns[mode].append((w1 - w0) * 1e9 / n)
    aa = abs(statistics.median(ns["detached"]) - statistics.median(ns["detached2"]))
    print(f"ppe_classify_flow_host, 65,536 packets (16,384 connections), pageable, chunk 0, wall ns per packet: "
          f"attached {fmt(ns['attached'])}  detached {fmt(ns['detached'])}  detached again {fmt(ns['detached2'])}  "
          f"A/A spread {aa:.2f}", flush=True)
    for e in engs.values():
        e.flow_destroy()
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024])
    a = ap.parse_args()
    classify_part(a)
    host_part(a)


if __name__ == "__main__":
    main()
