#!/usr/bin/env python3
"""Cost of the port-scan detector on the flow-table path (diagnostics): flow batches of 1 .. MAX 64-B
packets through ppe_classify_flow on an engine with a port-scan table flow-attached (the one-launch kernel with the
detector inside) and on a twin with nothing attached (today's kernels: the yardstick), the modes alternating in one
process, the same build.  Workloads:
  found      a warm table, every packet finds its flow (no packet reaches the detector)
  newflows   every packet a new flow from a source of its own (a different batch per call; the table is aged empty
             between the rounds)
  scan-quiet one source, a new port with every packet, nothing forwarded, a quiet previous window: every packet OK
  scan-hot   the same with the source held: every packet HOLD (status 24)
  mixed      tests/flow_portscan_model.py's generated batch (8 sources, 6 ports, both directions)
  pool-short the flow pool full: every would-be creator is FLOW_NOMEM, in index order (the kernel's worst case)

Per workload and size: --rounds rounds of --calls calls enqueued back to back on one stream; stream us per call (events
around the calls), median (min-max) over the rounds; the detached twin runs twice per round, and the spread between its
two medians is the run's A/A spread; `rounds` is the resolve phase's round count of the last attached batch.

Then PPE_FLOW_PS_MAX's candidates: a 65,536-packet pageable ppe_classify_flow_host call on the mixed workload in chunks
of 512 and 1,024 (what a maximum of 512 / 1,024 makes of it), wall ns per packet.  Then Decode (include/ppe_decode.h) at
bursts of 1 and 64 with flow_able 1 and flow_portscan_able 0, 1 and 0 again: wall us per flush.

  python tools/ab_flow_portscan.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024]
"""
import argparse
import ctypes as C
import statistics
import sys
import time
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
    """name -> (rules, default action, flow capacity, batches cycled over the calls, prime batch or None, aged)."""
    srv = 0x0B000001
    udp = lambda k: udp_packet(0x0A000000 + k, srv, 1024 + (k & 0x7FFF), 53)  # noqa: E731
    scan = stack([tcp_packet(0x0A000001, srv, 40000, 1000 + p, flags=0x02) for p in range(n)])
    none = np.zeros(0, abi.RULE_DTYPE)
    return {
        "found": (any_rule(), DROP, 1 << 16, [stack([udp(k) for k in range(n)])], None, False),
        "newflows": (any_rule(), DROP, 1 << 19, [stack([udp(c * n + k) for k in range(n)]) for c in range(calls)], None,
                     True),
        "scan-quiet": (none, DROP, 1 << 16, [scan], None, False),
        "scan-hot": (none, DROP, 1 << 16, [scan], stack([udp_packet(0x0A000001, srv, 5000, 100 + p) for p in range(5)]),
                     False),
        "mixed": (fpm.gen_rules(), DROP, 1 << 16, [fpm.gen_batch(np.random.default_rng(3), n)], None, False),
        "pool-short": (any_rule(), DROP, 1, [stack([udp(k) for k in range(n)])], None, False),
    }


def classify_part(a):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    print(f"ppe_classify_flow, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    for n in a.sizes:
        for name, (rules, dflt, cap, batches, prime, aged) in workloads(n, a.calls).items():
            engs, ps = {}, None
            for mode in ("attached", "detached"):
                e = engs[mode] = Engine(0)
                e.commit(rules, default_action=dflt)
                e.flow_create(cap, 2048)
            ps = engs["attached"].portscan(attach="flow", able=1, exception_freq=3, hold_seconds=600, capacity=1 << 19,
                                           max_batch=2048, cycles_per_second=RATE)
            ps.clock(10 * RATE, 1000)
            dv = [(torch.from_numpy(h).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev)) for h, ln in batches]
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
            if prime is not None:  # five ports in one window, then the window rolls: the next change is DETECTED
                th, tl = torch.from_numpy(prime[0]).to(dev), torch.from_numpy(prime[1].view(np.int32)).to(dev)
                po = {k: torch.empty(5, dtype=torch.int32, device=dev) for k in out}
                engs["attached"].classify_flow_torch(th, tl, po, cfg=engs["attached"].cfg(0, 1, 1000), stream=stream)
                torch.cuda.synchronize()
                ps.clock(11 * RATE + RATE // 2, 1001)
            modes = ("detached", "attached", "detached2")
            gpu = {m: [] for m in modes}
            rounds = 0
            for r in range(a.rounds + 1):  # round 0: warm-up (and the batch's flows enter both tables)
                for mode in modes:
                    e = engs["attached" if mode == "attached" else "detached"]
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
                    if mode == "attached":
                        rounds = e.flow_portscan_rounds()
            aa = abs(statistics.median(gpu["detached"]) - statistics.median(gpu["detached2"]))
            kinds = {m: engs[m].flow_launch_info() for m in engs}
            info = ps.info()
            print(f"n {n:5d} {name:>10}: attached {fmt(gpu['attached'])}  detached {fmt(gpu['detached'])}  "
                  f"detached again {fmt(gpu['detached2'])}  A/A spread {aa:.2f}  rounds {rounds}  "
                  f"[kind, launches: {kinds['attached']} / {kinds['detached']}; ok/nomem/detected/hold "
                  f"{info['ok']}/{info['nomem']}/{info['detected']}/{info['hold']}]", flush=True)
            ps.close()
            for e in engs.values():
                e.flow_destroy()
                e.close()


def max_part(a):
    """65,536 mixed packets, pageable, through ppe_classify_flow_host in chunks of 512 and 1,024."""
    n = 65536
    hdr, lens = fpm.gen_batch(np.random.default_rng(5), n)
    ts = np.full(n, 1000, np.uint64)
    e = Engine(0)
    e.commit(fpm.gen_rules(), default_action=DROP)
    e.flow_create(1 << 16, 4096)
    ps = e.portscan(attach="flow", able=1, exception_freq=3, hold_seconds=2, max_batch=4096, cycles_per_second=RATE)
    ns = {512: [], 1024: [], "1024 again": []}
    for r in range(a.rounds + 1):
        for key in (512, 1024, "1024 again"):
            ps.clock((10 + 3 * r) * RATE, 1000 + 3 * r)
            w0 = time.perf_counter()
            e.classify_flow_host(hdr, lens, ts, cfg=e.cfg(0, 1, 1000 + 3 * r), chunk=512 if key == 512 else 1024,
                                 outputs=("verdict", "flow_hash", "acl_hit"))
            w1 = time.perf_counter()
            if r:
                ns[key].append((w1 - w0) * 1e9 / n)
    aa = abs(statistics.median(ns[1024]) - statistics.median(ns["1024 again"]))
    print(f"ppe_classify_flow_host, 65,536 mixed packets, pageable, wall ns per packet: chunk 512 {fmt(ns[512])}  "
          f"chunk 1024 {fmt(ns[1024])}  chunk 1024 again {fmt(ns['1024 again'])}  A/A spread {aa:.2f}", flush=True)
    ps.close()
    e.flow_destroy()
    e.close()


def decode_part(a):
    rules = fpm.gen_rules()
    lib = abi.load()
    assert lib.DP_Acl_Rule_Init() == 0
    lib.ppe_rule_list_free()
    assert lib.ppe_rule_list_init() == 0
    for i in range(len(rules)):
        rid = C.c_uint32()
        assert lib.Rule_add(rules[i:i + 1].ctypes.data, C.byref(rid)) == 0
    dflt = C.c_uint32.in_dll(lib, "dp_acl_action_default")
    old = dflt.value
    dflt.value = DROP
    assert lib.DP_Acl_Rule_Commit() == 0
    flow, fps = C.c_uint32.in_dll(lib, "flow_able"), C.c_uint32.in_dll(lib, "flow_portscan_able")
    flow.value = 1
    calls = max(1, a.calls // 4)
    print(f"Decode, flow_able 1, {a.rounds} rounds x {calls} flushes, wall us per flush: median (min-max)")
    for burst in (1, 64):
        hdr, lens = fpm.gen_batch(np.random.default_rng(7), burst, stride=144)
        bufs = [C.create_string_buffer(bytes(hdr[i]), 144) for i in range(burst)]
        mbufs = (abi.Mbuf * burst)()
        for i in range(burst):
            mbufs[i].pkt_ptr = C.cast(bufs[i], C.c_void_p)
            mbufs[i].pkt_totallen = int(lens[i])
            mbufs[i].timestamp = 1000
        refs = [C.byref(mbufs[i]) for i in range(burst)]
        lib.Decode_Set_Burst(burst)
        modes = (("flow_portscan_able 0", 0), ("flow_portscan_able 1", 1), ("flow_portscan_able 0 again", 0))
        us = {m: [] for m, _ in modes}
        for r in range(a.rounds + 1):
            for m, v in modes:
                fps.value = v
                lib.DP_Flow_Clock(1000 + r)
                lib.DP_PortScan_Clock((10 + r) * 10**9, 1000 + r)
                w0 = time.perf_counter()
                for _ in range(calls):
                    for ref in refs:
                        lib.Decode(ref)       # the burst's last Decode classifies and delivers it
                w1 = time.perf_counter()
                if r:
                    us[m].append((w1 - w0) * 1e6 / calls)
        aa = abs(statistics.median(us[modes[0][0]]) - statistics.median(us[modes[2][0]]))
        print(f"burst {burst:3d}: " + "  ".join(f"{m} {fmt(us[m])}" for m, _ in modes) + f"  A/A spread {aa:.2f}",
              flush=True)
    flow.value = fps.value = 0
    dflt.value = old
    lib.Decode_Set_Burst(1)
    lib.ppe_rule_list_free()
    lib.DP_Acl_Rule_Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024])
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    classify_part(a)
    max_part(a)
    if not a.no_decode:
        decode_part(a)


if __name__ == "__main__":
    main()
