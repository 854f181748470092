#!/usr/bin/env python3
"""Cost of a ppe_defrag batch on small batches (diagnostics; fixes PPE_DEFRAG_SMALL_CUTOFF): batches of
1 .. 256 fragments through ppe_defrag on a table that takes the one-launch kernel at every size its workgroup holds
(created under PPE_DEFRAG_SMALL=256, so sizes past the cutoff in force are measured too) and on a table created under
PPE_DEFRAG_SMALL=0 (the six launches: the yardstick, the code as it was), the modes alternating in one process, the
same build.

Workloads, each --calls different batches of n fragments per round:
  new       every fragment starts a new datagram (a creator: claim, admission, a fresh FCB, a stash);
  complete  every fragment completes a datagram whose head an earlier (untimed) batch left in the table (found in the
            table, the chain read from the store slot, one assembly per fragment);
  mix       consecutive slices of synth.make_fragment_stream.
Before every timed run the table is aged empty, so every mode of a round sees the same table.

Per size, workload and mode: --rounds rounds of --calls calls enqueued back to back on one stream; the figure is the
stream time per call (events around the calls).  Median (min-max) over the rounds; the six-launch mode runs twice per
round, and the spread between its two medians is the run's A/A spread.  A size supports the one-launch kernel when, on
every workload, its median is not above the six launches' (the lower of the two) by more than that spread; the cutoff
is the largest measured size up to which every measured size does.

Then the same through Decode (include/ppe_decode.h) at bursts of 1 and 64 of pure fragments (two-fragment datagrams: a
burst of 1 alternates heads and tails, a burst of 64 carries 32 of each) with defrag_able 0, 1 and 0 again: wall
microseconds per flush, no hooks set; an untimed DP_Defrag_Age every 16 flushes frees the completed FCBs.

  python tools/ab_defrag_small.py [--calls 200] [--rounds 5] [--sizes 1,2,4,8,64,256] [--no-decode]
"""
import argparse
import ctypes as C
import os
import time
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle"), str(ROOT / "tests"), str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pktbuild import arena, ip_frag  # noqa: E402
from ppe import Defrag, Engine, abi, synth  # noqa: E402

NOW = 1_700_000_000
PAY = bytes(range(64))


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f}-{max(v):.2f})"


def workload(kind, n, calls):
    """(arena, off, len, setup): call k's batch is fragments [k n, (k + 1) n); setup: fragments of an untimed batch
    run first (the heads the `complete` fragments finish), or None."""
    if kind == "mix":
        a, o, l = synth.make_fragment_stream(max(64, int(n * calls / 3.0) + 64), seed=5)
        assert len(l) >= n * calls
        return a, o[:n * calls], l[:n * calls], None
    heads, tails = [], []
    for k in range(calls):
        for i in range(n):
            s, d = 0x0A000000 + i, 0x0B000000 + k
            heads.append(ip_frag(17, s, d, 7, 0, True, PAY[:32]))
            tails.append(ip_frag(17, s, d, 7, 32, False, PAY[32:]))
    if kind == "new":
        return (*arena(heads), None)
    a, o, l = arena(tails + heads)
    m = n * calls
    return a, o[:m], l[:m], (o[m:], l[m:])


def measure(a):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    eng = Engine(0)
    nmax = max(a.sizes)
    tabs = {}
    for mode in ("one", "six"):
        os.environ["PPE_DEFRAG_SMALL"] = "0" if mode == "six" else "256"
        try:
            tabs[mode] = Defrag(eng, fcb_max=1 << 16, max_batch=max(1 << 16, nmax))
        finally:
            os.environ.pop("PPE_DEFRAG_SMALL", None)
    modes = ("six", "one", "six2")
    print(f"ppe_defrag, {a.rounds} rounds x {a.calls} calls, stream us per call: median (min-max)")
    supported, clock = {}, NOW
    for n in a.sizes:
        supported[n] = True
        for kind in ("new", "complete", "mix"):
            ar, off, lens, setup = workload(kind, n, a.calls)
            ta = torch.from_numpy(ar).to(dev)
            to = torch.from_numpy(off.view(np.int64)).to(dev)
            tl = torch.from_numpy(lens.view(np.int32)).to(dev)
            if setup is not None:
                so = torch.from_numpy(setup[0].view(np.int64)).to(dev)
                sl = torch.from_numpy(setup[1].view(np.int32)).to(dev)
            us = {m: [] for m in modes}
            delta, before = {}, {m: tabs[m].info() for m in tabs}
            outs = {m: tabs[m].alloc_out(n, 128) for m in tabs}
            big = {m: tabs[m].alloc_out(n * a.calls, 128, full=False) for m in tabs} if setup is not None else None
            for r in range(a.rounds + 1):   # round 0: warm-up
                for mode in modes:
                    key = "one" if mode == "one" else "six"
                    t = tabs[key]
                    clock += 1000
                    t.age(clock, 20)        # everything the last run left is idle: an empty table
                    if setup is not None:
                        for b in range(0, n * a.calls, 1 << 16):
                            t.run_torch(ta, so[b:b + (1 << 16)], sl[b:b + (1 << 16)], big[key], clock,
                                        stream=stream)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(stream)
                    for k in range(a.calls):
                        t.run_torch(ta, to[k * n:(k + 1) * n], tl[k * n:(k + 1) * n], outs[key], clock,
                                    stream=stream)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if r:
                        us[mode].append(e0.elapsed_time(e1) * 1e3 / a.calls)
                    after = t.info()        # (outside the timed region) what the run counted: the same in every mode
                    delta[mode] = {k: after[k] - before[key].get(k, 0) for k in after if k.startswith("st_")}
                    before[key] = after
                assert delta["one"] == delta["six"] == delta["six2"], f"the tables disagree: {delta}"
            kinds = {m: tabs[m].launch_info() for m in tabs}
            aa = abs(statistics.median(us["six"]) - statistics.median(us["six2"]))
            six = min(statistics.median(us["six"]), statistics.median(us["six2"]))
            ok = statistics.median(us["one"]) <= six + aa
            supported[n] = supported[n] and ok
            print(f"n {n:4d} {kind:>8}: one launch {fmt(us['one'])}  six launches {fmt(us['six'])}  "
                  f"six again {fmt(us['six2'])}  A/A spread {aa:.2f}  one launch {'not slower' if ok else 'SLOWER'}"
                  f"  [kind, launches: {kinds['one']} / {kinds['six']}]", flush=True)
    best = 0
    for n in a.sizes:
        if not supported[n]:
            break
        best = n
    print(f"largest measured size up to which the one-launch kernel is supported on every workload: {best}", flush=True)
    for t in tabs.values():
        t.close()
    eng.close()


def decode_part(a):
    lib = abi.load()
    assert lib.DP_Acl_Rule_Init() == 0
    lib.ppe_rule_list_free()
    assert lib.ppe_rule_list_init() == 0
    dflt = C.c_uint32.in_dll(lib, "dp_acl_action_default")
    old = dflt.value
    dflt.value = 0
    assert lib.DP_Acl_Rule_Commit() == 0
    able = C.c_uint32.in_dll(lib, "defrag_able")
    calls = max(16, a.calls // 4 // 16 * 16)
    print(f"Decode, pure fragments, {a.rounds} rounds x {calls} flushes, wall us per flush: median (min-max)")
    for burst in (1, 64):
        # 16 variants of the burst (the ip_id differs), so no key repeats between two aging calls
        variants = []
        for v in range(16):
            frames = []
            for i in range(max(1, burst // 2)):
                s, d = 0x0A000000 + i, 0x0B000000
                frames += [ip_frag(17, s, d, 100 + v, 0, True, PAY[:32]), ip_frag(17, s, d, 100 + v, 32, False, PAY[32:])]
            bufs = [C.create_string_buffer(f, len(f) + 8) for f in frames]
            mb = (abi.Mbuf * len(frames))()
            for i, f in enumerate(frames):
                mb[i].pkt_ptr = C.cast(bufs[i], C.c_void_p).value
                mb[i].pkt_totallen = len(f)
            variants.append((bufs, mb, [C.byref(mb[i]) for i in range(len(frames))]))
        lib.Decode_Set_Burst(burst)
        modes = (("defrag_able 0", 0), ("defrag_able 1", 1), ("defrag_able 0 again", 0))
        us = {m: [] for m, _ in modes}
        now = NOW
        for r in range(a.rounds + 1):
            for m, val in modes:
                able.value = val
                total = 0.0
                for k in range(calls):
                    refs = variants[k % 16][2]
                    lib.DP_Defrag_Clock(now)
                    w0 = time.perf_counter()
                    for ref in refs:
                        lib.Decode(ref)       # at burst 1 every Decode is a flush; at 64 the last one
                    total += time.perf_counter() - w0
                    if k % 16 == 15:
                        now += 100
                        lib.DP_Defrag_Age(now, None)
                flushes = calls * (2 if burst == 1 else 1)
                if r:
                    us[m].append(total * 1e6 / flushes)
        aa = abs(statistics.median(us["defrag_able 0"]) - statistics.median(us["defrag_able 0 again"]))
        print(f"burst {burst:3d}: " + "  ".join(f"{m} {fmt(us[m])}" for m, _ in modes) + f"  A/A spread {aa:.2f}",
              flush=True)
    fi = abi.DefragInfo()
    assert lib.ppe_defrag_info(C.c_void_p(lib.DP_Defrag_Table()), C.byref(fi)) == 0
    print("table after the run:", {k: v for k, v in fi.as_dict().items() if k.startswith("st_") and v}, flush=True)
    able.value = 0
    dflt.value = old
    lib.Decode_Set_Burst(1)
    lib.ppe_rule_list_free()
    lib.DP_Acl_Rule_Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[1, 2, 4, 8, 64, 256])
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    if not a.no_kernel:
        measure(a)
    if not a.no_decode:
        decode_part(a)


if __name__ == "__main__":
    main()
