#!/usr/bin/env python3
"""Cost of a flow batch on small batches (diagnostics; fixes PPE_FLOW_SMALL_CUTOFF): C1's rule set,
F1's flow population cut to the size under test (one flow per four packets, both directions, a warm table), batches of
1 .. 4,096 64-B packets through ppe_classify_flow on a table that takes the one-launch kernel, on a table created under
PPE_FLOW_SMALL=0 (the two launches: the yardstick, the code as it was), and through the stateless ppe_classify of the same
packets (the floor), the modes alternating in one process, the same build.

Per size and mode: --rounds rounds of --calls calls enqueued back to back on one stream; `gpu` is the stream time per
call (events around the calls), `wall` the host time per call including the final synchronise.  Median (min-max) over the
rounds; the two-launch mode runs twice per round, and the spread between its two medians is the run's A/A spread.  A
size supports the one-launch kernel when its gpu median is not above the two launches' by more than that spread; the
cutoff is the largest measured size, at most 2,048, up to which every measured size does.

Then the same through Decode (include/ppe_decode.h) at bursts of 1, 64 and 512 with flow_able 0, 1 and 0 again: wall
microseconds per flush.

  python tools/ab_flow_small.py [--calls 200] [--rounds 5] [--sizes 1,64,512,1024,2048,4096]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppe import Engine, abi, synth  # noqa: E402

NOW = 1_700_000_000


def packets(n, rules, seed=11):
    pk = synth.make_flow_packets(n, rules, n_flows=max(1, n // 4), seed=seed, template_seed=5, kind="udp64", stride=64)
    return pk["hdr"], pk["len"]


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f}-{max(v):.2f})"


def classify_part(a, rules):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    nmax = max(a.sizes)
    engs = {}
    for mode in ("one", "two"):
        engs[mode] = Engine(0)
        engs[mode].commit(rules, default_action=0)
        if mode == "two":
            os.environ["PPE_FLOW_SMALL"] = "0"
        try:
            engs[mode].flow_create(1 << 16, max(nmax, 64))
        finally:
            os.environ.pop("PPE_FLOW_SMALL", None)
    modes = ("two", "one", "stateless", "two2")
    print(f"ppe_classify_flow, C1 rules, {a.rounds} rounds x {a.calls} calls, us per call: median (min-max)")
    supported = []
    for n in a.sizes:
        hdr, lens = packets(n, rules)
        th = torch.from_numpy(hdr).to(dev)
        tl = torch.from_numpy(lens.view(np.int32)).to(dev)
        out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("verdict", "flow_hash", "acl_hit")}
        gpu, wall = {m: [] for m in modes}, {m: [] for m in modes}
        for r in range(a.rounds + 1):  # round 0: warm-up (and the batch's flows enter both tables)
            for mode in modes:
                eng = engs["one" if mode in ("one", "stateless") else "two"]
                cfg = eng.cfg(now_seconds=NOW + r)
                call = eng.classify_torch if mode == "stateless" else eng.classify_flow_torch
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record(stream)
                for _ in range(a.calls):
                    call(th, tl, out, cfg=cfg, stream=stream)
                e1.record(stream)
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                if r:
                    gpu[mode].append(e0.elapsed_time(e1) * 1e3 / a.calls)
                    wall[mode].append((w1 - w0) * 1e6 / a.calls)
        kinds = {m: engs[m].flow_launch_info() for m in engs}
        for what, us in (("gpu", gpu), ("wall", wall)):
            aa = abs(statistics.median(us["two"]) - statistics.median(us["two2"]))
            two = min(statistics.median(us["two"]), statistics.median(us["two2"]))
            ok = statistics.median(us["one"]) <= two + aa
            if what == "gpu":
                supported.append((n, ok))
            print(f"n {n:5d} {what:>4}: one launch {fmt(us['one'])}  two launches {fmt(us['two'])}  "
                  f"two again {fmt(us['two2'])}  stateless {fmt(us['stateless'])}  A/A spread {aa:.2f}  "
                  f"one launch {'not slower' if ok else 'SLOWER'}"
                  + (f"  [kind, launches: {kinds['one']} / {kinds['two']}]" if what == "gpu" else ""), flush=True)
    best = 0
    for n, ok in supported:
        if not ok:
            break
        if n <= 2048:
            best = n
    print(f"largest measured size up to which the one-launch kernel is supported (<= 2,048): {best}", flush=True)
    for e in engs.values():
        e.flow_destroy()
        e.close()


def decode_part(a, rules):
    lib = abi.load()
    assert lib.DP_Acl_Rule_Init() == 0
    lib.ppe_rule_list_free()
    assert lib.ppe_rule_list_init() == 0
    for i in range(len(rules)):
        rid = C.c_uint32()
        assert lib.Rule_add(rules[i:i + 1].ctypes.data, C.byref(rid)) == 0
    dflt = C.c_uint32.in_dll(lib, "dp_acl_action_default")
    old = dflt.value
    dflt.value = 0
    assert lib.DP_Acl_Rule_Commit() == 0
    able = C.c_uint32.in_dll(lib, "flow_able")
    calls = max(1, a.calls // 4)
    print(f"Decode, C1 rules, {a.rounds} rounds x {calls} flushes, wall us per flush: median (min-max)")
    for burst in (1, 64, 512):
        hdr, lens = packets(burst, rules)
        bufs = [C.create_string_buffer(bytes(hdr[i]), 144) for i in range(burst)]
        mbufs = (abi.Mbuf * burst)()
        for i in range(burst):
            mbufs[i].pkt_ptr = C.cast(bufs[i], C.c_void_p)
            mbufs[i].pkt_totallen = int(lens[i])
            mbufs[i].timestamp = NOW
        refs = [C.byref(mbufs[i]) for i in range(burst)]
        lib.Decode_Set_Burst(burst)
        modes = (("flow_able 0", 0), ("flow_able 1", 1), ("flow_able 0 again", 0))
        us = {m: [] for m, _ in modes}
        for r in range(a.rounds + 1):
            for m, v in modes:
                able.value = v
                lib.DP_Flow_Clock(NOW + r)
                w0 = time.perf_counter()
                for _ in range(calls):
                    for ref in refs:
                        lib.Decode(ref)       # the burst's last Decode classifies and delivers it
                w1 = time.perf_counter()
                if r:
                    us[m].append((w1 - w0) * 1e6 / calls)
        aa = abs(statistics.median(us["flow_able 0"]) - statistics.median(us["flow_able 0 again"]))
        print(f"burst {burst:3d}: " + "  ".join(f"{m} {fmt(us[m])}" for m, _ in modes) + f"  A/A spread {aa:.2f}",
              flush=True)
    able.value = 0
    dflt.value = old
    lib.Decode_Set_Burst(1)
    lib.ppe_rule_list_free()
    lib.DP_Acl_Rule_Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 1024, 2048, 4096])
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    rules = synth.make_rules(synth.CONFIGS["C1"]["rules"])
    classify_part(a, rules)
    if not a.no_decode:
        decode_part(a, rules)


if __name__ == "__main__":
    main()
