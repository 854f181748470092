#!/usr/bin/env python3
"""Cost of the monitors on host flow batches and behind Decode (diagnostics).

1. Kind 4 against two launches.  Flow batches of n 64-B packets through ppe_classify_flow_host_ports' zero-copy form
   (every buffer pinned, the port bytes too) on an engine with all-zero monitor rules flow-attached (one launch,
   ppe_flow_launch_info kind 4) and on a twin whose table was created under PPE_FLOW_SMALL=0 (the two launches, kind 0:
   the yardstick), the modes alternating in one process, the same build.  The call synchronises its internal stream
   before it returns, so calls cannot be enqueued back to back and no event can be placed on that stream from outside:
   the figure is the wall time of the call, entry to return, which is the stream's time plus the submission and the
   wake-up, equal on both sides.  Workloads:
     found      a warm table, every packet finds its flow
     newflows   every packet a TCP SYN of a new flow (a different batch per call; the table is aged empty between the
                rounds): every packet a creator counted in syncount_accum
     mixed      tests/flow_portscan_model.py's generated batch (8 sources, 6 ports, both directions)
   (A size above PPE_FLOW_SMALL_ATK_CUTOFF takes the two launches on both sides: to measure the one launch there, build
   with -DPPE_FLOW_SMALL_ATK_CUTOFF=512u, as the measurement that set the bound did.)
   Per workload and size: --rounds rounds of --calls calls; us per call, median (min-max) over the rounds; the twin runs
   twice per round, and the spread between its two medians is the run's A/A spread.
2. Cost of the monitors on the host path: one staged call of 65,536 pageable packets, wall ns per packet, all-zero rules
   flow-attached against nothing attached (measured twice).
3. Decode per flush at bursts of 1 and 64 with flow_able 1 and flow_attack_able 0, 1 and 0 again: wall us per flush.

  python tools/ab_flow_host_ports.py [--calls 200] [--rounds 5] [--sizes 1,64,256] [--workloads found,newflows,mixed]
                                     [--no-staged] [--no-decode]
"""
import argparse
import ctypes as C
import os
import re
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

FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
CUTOFF = int(re.search(r"#define PPE_FLOW_SMALL_ATK_CUTOFF (\d+)u",
                       (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()).group(1))


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


def pin(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).pin_memory()


def kind_part(a):
    print(f"ppe_classify_flow_host_ports, zero-copy, {a.rounds} rounds x {a.calls} calls, wall us per call: median (min-max)")
    for n in a.sizes:
        for name, (rules, dflt, cap, batches, aged) in workloads(n, a.calls).items():
            if name not in a.workloads:
                continue
            engs, atks = {}, {}
            for mode in ("one", "two"):
                e = engs[mode] = Engine(0)
                e.commit(rules, default_action=dflt)
                if mode == "two":
                    os.environ["PPE_FLOW_SMALL"] = "0"   # read when the table is created
                try:
                    e.flow_create(cap, 2048)
                finally:
                    os.environ.pop("PPE_FLOW_SMALL", None)
                atks[mode] = e.attack(attach="flow")     # all-zero rules: the monitors count and drop nothing
                atks[mode].clock(1000)
            ports = pin((np.arange(n) % 4).astype(np.uint8), np.uint8)
            hb = [(pin(h, np.uint8), pin(ln, np.int32)) for h, ln in batches]
            out = {k: torch.empty(n, dtype=torch.int32).pin_memory() for k in ("verdict", "flow_hash", "acl_hit")}
            modes = ("two", "one", "two again")
            us = {m: [] for m in modes}
            for r in range(a.rounds + 1):  # round 0: warm-up (and the batch's flows enter both tables)
                for mode in modes:
                    key = "one" if mode == "one" else "two"
                    e = engs[key]
                    now = 1001
                    if aged and r:
                        now = 1001 + 100 * (3 * r + modes.index(mode))
                        e.flow_age(now, 1)
                    cfg = e.cfg(0, 1, now)
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    for c in range(a.calls):
                        th, tl = hb[c % len(hb)]
                        e.classify_flow_host_ports(th, tl, ports, cfg=cfg, out=out)
                    w1 = time.perf_counter()
                    if r:
                        us[mode].append((w1 - w0) * 1e6 / a.calls)
                    atks[key].tick(1001 + r)
            aa = abs(statistics.median(us["two"]) - statistics.median(us["two again"]))
            best = min(statistics.median(us["two"]), statistics.median(us["two again"]))
            d = statistics.median(us["one"]) - best
            kinds = {m: engs[m].flow_launch_info() for m in engs}
            print(f"n {n:5d} {name:>9}: one launch {fmt(us['one'])}  two launches {fmt(us['two'])}  "
                  f"two launches again {fmt(us['two again'])}  A/A spread {aa:.2f}  one - two {d:+.2f}  "
                  f"[kind, launches: {kinds['one']} / {kinds['two']}]", flush=True)
            for m in engs:
                atks[m].close()
                engs[m].flow_destroy()
                engs[m].close()


def staged_part(a):
    """65,536 mixed packets, pageable, one staged call: all-zero rules flow-attached against nothing attached."""
    n = 65536
    hdr, lens = fpm.gen_batch(np.random.default_rng(5), n)
    ports = (np.arange(n) % 4).astype(np.uint8)
    e = Engine(0)
    e.commit(fpm.gen_rules(), default_action=DROP)
    e.flow_create(1 << 17, 1 << 16)
    atk = e.attack(attach=False)
    atk.clock(1000)
    modes = ("nothing", "attached", "nothing again")
    ns = {m: [] for m in modes}
    for r in range(a.rounds + 1):
        for m in modes:
            if m == "attached":
                atk.attach_flow()
            w0 = time.perf_counter()
            e.classify_flow_host_ports(hdr, lens, ports, cfg=e.cfg(0, 1, 1000 + r), outputs=("verdict", "flow_hash", "acl_hit"))
            w1 = time.perf_counter()
            if m == "attached":
                atk.tick(1001 + r)
                atk.detach_flow()
            if r:
                ns[m].append((w1 - w0) * 1e9 / n)
    aa = abs(statistics.median(ns["nothing"]) - statistics.median(ns["nothing again"]))
    print("ppe_classify_flow_host_ports, 65,536 mixed packets, pageable, staged, wall ns per packet: "
          + "  ".join(f"{m} {fmt(ns[m])}" for m in modes) + f"  A/A spread {aa:.2f}", flush=True)
    atk.close()
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
    flow, fatk = C.c_uint32.in_dll(lib, "flow_able"), C.c_uint32.in_dll(lib, "flow_attack_able")
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
            mbufs[i].input_port = i % 4
        refs = [C.byref(mbufs[i]) for i in range(burst)]
        lib.Decode_Set_Burst(burst)
        modes = (("flow_attack_able 0", 0), ("flow_attack_able 1", 1), ("flow_attack_able 0 again", 0))
        us = {m: [] for m, _ in modes}
        for r in range(a.rounds + 1):
            for m, v in modes:
                fatk.value = v
                lib.DP_Flow_Clock(1000 + r)
                lib.DP_Attack_Tick(1000 + r)
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
    flow.value = fatk.value = 0
    dflt.value = old
    lib.Decode_Set_Burst(1)
    lib.ppe_rule_list_free()
    lib.DP_Acl_Rule_Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, CUTOFF])
    ap.add_argument("--workloads", type=lambda s: s.split(","), default=["found", "newflows", "mixed"])
    ap.add_argument("--no-staged", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    kind_part(a)
    if not a.no_staged:
        staged_part(a)
    if not a.no_decode:
        decode_part(a)


if __name__ == "__main__":
    main()
