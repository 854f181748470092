#!/usr/bin/env python3
"""Cost of the port-scan pre-pass on small batches (diagnostics): C1's rule set, batches of 1 .. 4,096 64-B packets
through ppe_classify with the table detached, attached with the one-launch pre-pass, and attached with a table created
under PPE_PS_FUSED=0 (the staged launches), the modes alternating in one process, the same build.

Per size and mode: --rounds rounds of --calls calls enqueued back to back on one stream; `gpu` is the stream time per
call (events around the calls), `wall` the host time per call including the final synchronise (what a caller that
enqueues and waits sees: the staged pre-pass is ten launches to enqueue).  Median (min-max) over the rounds; the
detached mode runs twice per round, and the spread between its two medians is the run's A/A spread.

Then ppe_classify_host_ordered from pageable buffers with the copies on the staging slots' streams and on the one
compute stream (PPE_HOST_ORDERED_COPY, read at context creation: two contexts), wall microseconds per call.

Then the same through Decode (include/ppe_decode.h) at burst 1 and burst 64 with portscan_able 0, 0 again and 1: wall
microseconds per Decode call (burst 1) or per burst of 64.

  python tools/ab_portscan_small.py [--calls 200] [--rounds 5] [--sizes 1,64,512,2048,4096]
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
RATE = 10**9


def packets(n, rules):
    """n 64-B UDP packets, every packet its own source address (each gets a record: 4,096 < 100,000)."""
    pk = synth.make_packets(n, rules, kind="udp64", stride=64, malformed_frac=0.0)
    hdr = pk["hdr"].copy()
    sip = (0x0B000000 + np.arange(n)).astype(np.uint32)
    for k in range(4):
        hdr[:, 26 + k] = (sip >> (24 - 8 * k)) & 0xFF
    return hdr, pk["len"]


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f}-{max(v):.2f})"


def classify_part(a, rules):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    eng = Engine(0)
    eng.commit(rules, default_action=1)
    nmax = max(a.sizes)
    tables = {"fused": eng.portscan(attach=False, max_batch=nmax)}
    os.environ["PPE_PS_FUSED"] = "0"
    try:
        tables["staged"] = eng.portscan(attach=False, max_batch=nmax)
    finally:
        del os.environ["PPE_PS_FUSED"]
    cfg = eng.cfg(now_seconds=NOW)
    modes = ("detached", "fused", "staged", "detached2")
    print(f"ppe_classify, C1 rules, {a.rounds} rounds x {a.calls} calls, us per call: median (min-max)")
    for n in a.sizes:
        hdr, lens = packets(n, rules)
        th = torch.from_numpy(hdr).to(dev)
        tl = torch.from_numpy(lens.view(np.int32)).to(dev)
        out = {"packed": torch.empty(n, dtype=torch.int64, device=dev), "part8": torch.empty(n, dtype=torch.uint8, device=dev)}
        gpu, wall = {m: [] for m in modes}, {m: [] for m in modes}
        for r in range(a.rounds + 1):  # round 0: warm-up
            for mode in modes:
                t = tables.get(mode)
                if t is not None:
                    t.clock((r + 2) * 100 * RATE + 1, NOW + r)
                    t.attach()
                elif getattr(eng, "portscan_attached", None) is not None:
                    eng.portscan_attached.detach()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record(stream)
                for _ in range(a.calls):
                    eng.classify_torch(th, tl, out, cfg=cfg, stream=stream)
                e1.record(stream)
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                if r:
                    gpu[mode].append(e0.elapsed_time(e1) * 1e3 / a.calls)
                    wall[mode].append((w1 - w0) * 1e6 / a.calls)
        if getattr(eng, "portscan_attached", None) is not None:
            eng.portscan_attached.detach()
        kinds = {m: tables[m].prepass_info() for m in tables}
        for what, us in (("gpu", gpu), ("wall", wall)):
            aa = abs(statistics.median(us["detached"]) - statistics.median(us["detached2"]))
            print(f"n {n:5d} {what:>4}: detached {fmt(us['detached'])}  fused {fmt(us['fused'])}  staged {fmt(us['staged'])}  "
                  f"detached again {fmt(us['detached2'])}  A/A spread {aa:.2f}"
                  + (f"  [pre-pass kind, launches: fused table {kinds['fused']}, staged table {kinds['staged']}]"
                     if what == "gpu" else ""), flush=True)
    for t in tables.values():
        t.close()
    eng.close()


def host_part(a, rules):
    print(f"ppe_classify_host_ordered, table attached, pageable buffers, {a.rounds} rounds x 20 calls, wall us per call")
    engs = {}
    for copy in ("1", "0"):
        os.environ["PPE_HOST_ORDERED_COPY"] = copy
        try:
            engs[copy] = Engine(0)
        finally:
            del os.environ["PPE_HOST_ORDERED_COPY"]
        engs[copy].commit(rules, default_action=1)
        engs[copy].portscan(max_batch=1 << 16).clock(200 * RATE, NOW)
    for n, chunk in ((64, 0), (4096, 1024), (1 << 18, 1 << 14), (1 << 18, 1 << 16)):
        hdr, lens = packets(n, rules)
        us = {c: [] for c in engs}
        for r in range(a.rounds + 1):
            for c, eng in engs.items():
                w0 = time.perf_counter()
                for _ in range(20):
                    eng.classify_host_ordered(hdr, lens, cfg=eng.cfg(now_seconds=NOW), chunk=chunk)
                if r:
                    us[c].append((time.perf_counter() - w0) * 1e6 / 20)
        print(f"n {n:7d} chunk {chunk:6d}: copies on the slots' streams {fmt(us['1'])}  on the compute stream {fmt(us['0'])}",
              flush=True)
    for eng in engs.values():
        eng.portscan_attached.close()
        eng.close()


def decode_part(a, rules):
    lib = abi.load()
    assert lib.DP_Acl_Rule_Init() == 0
    lib.ppe_rule_list_free()
    assert lib.ppe_rule_list_init() == 0
    for i in range(len(rules)):
        rid = C.c_uint32()
        assert lib.Rule_add(rules[i:i + 1].ctypes.data, C.byref(rid)) == 0
    assert lib.DP_Acl_Rule_Commit() == 0
    able = C.c_uint32.in_dll(lib, "portscan_able")
    print(f"Decode, C1 rules, {a.rounds} rounds x {a.calls} calls, wall us per call: median (min-max)")
    for burst in (1, 64):
        hdr, lens = packets(burst, rules)
        bufs = [C.create_string_buffer(bytes(hdr[i]), 144) for i in range(burst)]
        mbufs = (abi.Mbuf * burst)()
        for i in range(burst):
            mbufs[i].pkt_ptr = C.cast(bufs[i], C.c_void_p)
            mbufs[i].pkt_totallen = int(lens[i])
            mbufs[i].timestamp = NOW
        refs = [C.byref(mbufs[i]) for i in range(burst)]
        lib.Decode_Set_Burst(burst)
        modes = (("able 0", 0), ("able 1", 1), ("able 0 again", 0))
        us = {m: [] for m, _ in modes}
        for r in range(a.rounds + 1):
            for m, v in modes:
                able.value = v
                lib.DP_PortScan_Clock((r + 2) * 100 * RATE + 1, NOW + r)
                w0 = time.perf_counter()
                for _ in range(a.calls):
                    for ref in refs:
                        lib.Decode(ref)       # the burst's last Decode classifies and delivers it
                w1 = time.perf_counter()
                if r:
                    us[m].append((w1 - w0) * 1e6 / a.calls)
        aa = abs(statistics.median(us["able 0"]) - statistics.median(us["able 0 again"]))
        print(f"burst {burst:3d}: " + "  ".join(f"{m} {fmt(us[m])}" for m, _ in modes) + f"  A/A spread {aa:.2f}",
              flush=True)
    able.value = 0
    lib.Decode_Set_Burst(1)
    lib.ppe_rule_list_free()
    lib.DP_Acl_Rule_Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512, 2048, 4096])
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    rules = synth.make_rules(synth.CONFIGS["C1"]["rules"])
    classify_part(a, rules)
    if not a.no_decode:
        host_part(a, rules)
        decode_part(a, rules)


if __name__ == "__main__":
    main()
