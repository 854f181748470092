"""ppe_classify_flow_host_ports on the GPU: the flow-attached attack monitors on host-resident flow batches, whatever the
chunk size, and the one-launch kernel with the monitors in it (csrc/ppe_kernels_flow_small_attack.hip, launch kind 4).

After every call the verdict, ACL hit, flow hash and tuple, the 32 counters, ppe_attack_info, ppe_flow_info and the whole
dumped table must equal the serial model fed the WHOLE batch (tests/attack_flow_model.py; tests/flow_combined_model.py
for the monitors and the detector together), every output carries 64 guard entries that must stay untouched, and
ppe_flow_launch_info must name the path the last chunk took.  Integer work: no tolerance anywhere."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import test_flow_combined_model as tcm  # noqa: E402
from attack_model import batch, frame  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_attack import GUARD, PD, PLAIN, TD, collect, compare, mixed  # noqa: E402
from test_gpu_attack_flow import A, B, FLOOD0, FlowRig, accum, statuses  # noqa: E402
from test_gpu_flow import table  # noqa: E402
from test_gpu_flow_combined import Rig as CombinedRig, cbatch  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
INTERNAL = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()
CUTOFF = int(re.search(r"#define PPE_FLOW_SMALL_CUTOFF (\d+)u", INTERNAL).group(1))
# the largest chunk that takes the one launch with the monitors in it: the planner's own measured bound, at most CUTOFF
ACUT = int(re.search(r"#define PPE_FLOW_SMALL_ATK_CUTOFF (\d+)u", INTERNAL).group(1))
NOW = 1_700_000_000
DEV = torch.device("cuda:0")
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
FW, NOMEM = ST["ACL_FW"], ST["FLOW_NOMEM"]
SIZES = sorted({1, 63, 64, 65, ACUT - 1, ACUT, ACUT + 1, CUTOFF - 1, CUTOFF, CUTOFF + 1})
CHUNKS = tuple(dict.fromkeys((64, 128, ACUT, CUTOFF, 0)))


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "engines" in request.fixturenames:
        for e in request.getfixturevalue("engines"):
            for mark in ("attack_flow_attached", "attack_attached", "portscan_attached", "portscan_flow_attached"):
                if getattr(e, mark, None) is not None:
                    getattr(e, mark).close()
            e.stream_tcp(0, 0, 0)
            e.flow_combine(0)


def host_alloc(n, outs, pinned):
    """CPU buffers, pageable or pinned, each with 64 guard entries behind it (test_gpu_attack.collect checks them)."""
    out = {}
    for k in outs:
        t = torch.full(((4 * n if k == "tuple" else (n + 63) // 64 if k == "tile_cnt" else n) + GUARD,), -7,
                       dtype=torch.int64 if k == "packed" else torch.int32)
        if k == "part8":
            t = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8)
        out[k] = t.pin_memory() if pinned else t
    return out


def host_in(a, dtype, pinned):
    t = torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy())
    return t.pin_memory() if pinned else t


def ports_call(eng, hdr, lens, ports, out, cfg, chunk=0, pinned=False, pin_ports=None, ts=None, plain=False):
    """The raw call (plain: ppe_classify_flow_host instead); returns its code."""
    n = len(lens)
    th, tl = host_in(hdr, np.uint8, pinned), host_in(np.ascontiguousarray(lens, np.uint32), np.int32, pinned)
    tt = host_in(np.ascontiguousarray(ts, np.uint64), np.int64, pinned) if ts is not None else None
    tp = host_in(np.ascontiguousarray(ports, np.uint8), np.uint8, pinned if pin_ports is None else pin_ports) \
        if ports is not None else None
    g = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    b = abi.Batch(th.data_ptr(), tl.data_ptr(), tt.data_ptr() if tt is not None else None, n, hdr.shape[1])
    r = abi.Result(g("verdict"), g("flow_hash"), g("acl_hit"), g("fw_idx"), g("drop_idx"), g("tile_cnt"), g("tuple"),
                   g("part8"), g("packed"))
    if plain:
        return eng.lib.ppe_classify_flow_host(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), int(chunk))
    return eng.lib.ppe_classify_flow_host_ports(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), int(chunk),
                                                tp.data_ptr() if tp is not None else None)


def last_chunk(n, chunk, max_batch, zero_copy):
    """Packets in the call's last flow batch (include/ppe_hip.h: the chunk rounded up to 64 and clamped)."""
    if zero_copy and n <= max_batch:
        return n
    c = chunk or (1 << 18)
    c = min((c + 63) & ~63, max_batch & ~63, (n + 63) & ~63)
    return n - ((n - 1) // c) * c


class HostRig(FlowRig):
    """FlowRig whose batches go through ppe_classify_flow_host_ports: the model is still fed the whole batch."""
    chunk, pinned, pin_ports, max_batch = 0, False, None, 8192

    def __init__(self, eng, *a, **kw):
        self.max_batch = kw.get("max_batch", 8192)
        super().__init__(eng, *a, **kw)

    def classify(self, hdr, lens, ports, outs, now, syn_check):
        n = len(lens)
        out = host_alloc(n, PLAIN, self.pinned)
        rc = ports_call(self.eng, hdr, lens, ports, out, self.eng.cfg(0, syn_check, now), self.chunk, self.pinned,
                        self.pin_ports)
        assert rc == 0, (rc, self.eng.lib.ppe_last_error(self.eng.ctx))
        zc = self.pinned and (ports is None or self.pin_ports in (None, True))
        m = last_chunk(n, self.chunk, self.max_batch, zc)
        assert self.eng.flow_launch_info() == ((4, 1) if m <= ACUT else (0, 2)), (n, self.chunk, self.pinned, m)
        return collect(out, n)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_chunks_and_buffers(eng, n):
    """Every size at every chunk, pageable and pinned (pinned ports: the zero-copy form; pageable ports beside pinned
    buffers: the staged path), all four ports mixed in every tile, dropping rules on, a tick between the calls, a pool
    that runs out."""
    rig = HostRig(eng, pd=PD, td=TD, hold=2, capacity=max(4, n // 2))
    seen, k = set(), 0
    for chunk in CHUNKS:
        for pinned, pin_ports in ((False, None), (True, None), (True, False)):
            if pin_ports is False and chunk not in (64, 0):
                continue
            rig.chunk, rig.pinned, rig.pin_ports = chunk, pinned, pin_ports
            hdr, lens, ports = mixed(n, 100 * n + k % 5)
            _, e = rig.step(hdr, lens, ports, now=NOW + k, what=f"n {n} chunk {chunk} pinned {pinned}/{pin_ports}")
            seen |= set(statuses(e))
            k += 1
            rig.tick(NOW + k)
            if k == 5:
                rig.age(NOW + 40, 20)
    if n >= 63:
        assert {LAND, SYNF, UDPF, NOMEM, FW} <= seen, seen
    rig.close()


@pytest.mark.parametrize("n", SIZES)
def test_kind_four_against_the_two_launches(engines, n):
    """The same packets through the new call (zero-copy and staged: one launch, kind 4, up to its cutoff) and, on a twin
    context, through ppe_classify_flow with a sticky ppe_attack_ports array (two launches): outputs, counters, monitor
    state and table byte for byte."""
    rig = HostRig(engines[0], pd=PD, td=TD, hold=2, capacity=max(4, n // 2))
    twin = FlowRig(engines[1], pd=PD, td=TD, hold=2, capacity=max(4, n // 2))
    try:
        for k, pinned in enumerate((True, False, True)):
            rig.pinned = pinned
            hdr, lens, ports = mixed(n, 300 * n + k)
            got, _ = rig.step(hdr, lens, ports, now=NOW + k, what=f"n {n} call {k}")
            assert engines[0].flow_launch_info() == ((4, 1) if n <= ACUT else (0, 2))
            twin.eng.clear_counters()
            ref = twin.classify(hdr, lens, ports, PLAIN, NOW + k, 1)
            assert engines[1].flow_launch_info() == (0, 2)
            for name in PLAIN:
                assert got[name].tobytes() == ref[name].tobytes(), (name, k)
            assert engines[0].counters() == engines[1].counters()
            assert rig.atk.info() == twin.atk.info()
            assert table(engines[0].flow_dump()) == table(engines[1].flow_dump())
            f0, f1 = engines[0].flow_info(), engines[1].flow_info()
            assert all(f0[x] == f1[x] for x in ("live", "new_flow", "del_flow"))
            rig.tick(NOW + k + 1)
            twin.atk.tick(NOW + k + 1)
    finally:
        twin.m.close()
        twin.atk.close()
        engines[1].flow_destroy()
        rig.close()


@pytest.mark.parametrize("chunk", [64, 0])
def test_creator_and_dropped_syn_across_a_chunk_boundary(eng, chunk):
    """Port 0 drops every SYN (flood armed by the first interval), port 1 none.  One 5-tuple as creator and as dropped
    SYN on the two sides of 63 | 64, in both orders; at chunk 64 they are different flow batches."""
    rig = HostRig(eng, capacity=64, td={0: dict(FLOOD0, flood_udp=0)})
    rig.chunk = chunk
    rig.step(*batch([frame("syn", B, A)]), ports=np.zeros(1, np.uint8))
    rig.tick(NOW + 1)
    n = 130
    fr, ports = [frame("icmp", A + 50 + i, B) for i in range(n)], np.ones(n, np.uint8)
    place = {"W": (63, 64), "X": (65, 62), "Y": (5, 128), "Z": (129, 6)}       # tuple: (creator, dropped)
    for j, (cre, drp) in enumerate(place.values()):
        fr[cre] = fr[drp] = frame("syn", A + j, B)
        ports[drp] = 0
    _, e = rig.step(*batch(fr), ports=ports, now=NOW + 1)
    st = statuses(e)
    for cre, drp in place.values():
        assert st[cre] == FW and (int(e["verdict"][cre]) >> 16) & abi.F_NEWFLOW and st[drp] == SYNF
    fi = rig.check()
    assert fi["live"] == 5 and fi["tombstones"] == 0 and rig.m.atk.ai[1]["syncount_accum"] == 4
    rig.close()


def test_two_syns_of_one_tuple_in_different_chunks_on_different_ports(eng):
    """The creator (chunk 0, port 1) counts in syncount_accum; the later SYN (chunk 1, port 2) finds the flow: syn_accum
    only."""
    rig = HostRig(eng, capacity=64)
    rig.chunk = 64
    fr = [frame("icmp", A + 50 + i, B) for i in range(130)]
    ports = np.zeros(130, np.uint8)
    fr[10] = fr[100] = frame("syn", A, B)
    ports[10], ports[100] = 1, 2
    _, e = rig.step(*batch(fr), ports=ports)
    assert statuses(e)[10] == FW and statuses(e)[100] == FW
    assert (int(e["verdict"][10]) >> 16) & abi.F_NEWFLOW and not (int(e["verdict"][100]) >> 16) & abi.F_NEWFLOW
    assert accum(rig, 1) == (0, 1, 1) and accum(rig, 2) == (0, 1, 0) and accum(rig, 0) == (0, 0, 0)
    info = rig.atk.info()["ai"]
    assert [info[p]["syncount_accum"] for p in range(4)] == [0, 1, 0, 0]
    rig.close()


def test_udp_flood_arms_in_one_chunk_and_holds_the_next(eng):
    """udppps above the speed: the first UDP packet of the call lies in chunk 1 and arms the hold there, chunk 2's are
    dropped like it; two quiet ticks later the rate is 0 and the packets of the next call fall to the hold alone."""
    rig = HostRig(eng, capacity=64, td={0: dict(drop_pack=1, flood_udp=1, udp_speed=0)}, hold=50)
    rig.chunk = 64
    rig.step(*batch([frame("udp", A, B)]))
    rig.tick(NOW + 1)                                                  # udppps 1 > 0
    rig.clock(NOW + 1)
    fr = [frame("icmp", A + i, B) for i in range(64)] + [frame("udp", A, B)] * 128
    _, e = rig.step(*batch(fr), now=NOW + 1)
    assert statuses(e)[64:] == [UDPF] * 128
    a = rig.atk.info()["ai"][0]
    assert (a["udp_flood_hold"], a["udp_flood_hold_time"], a["udp_accum"]) == (1, NOW + 51, 128)
    rig.tick(NOW + 2)
    rig.tick(NOW + 3)                                                  # udppps 0, the hold stays until NOW + 51
    _, e = rig.step(*batch([frame("icmp", A, B)] * 64 + [frame("udp", A, B)] * 3), now=NOW + 3)
    assert statuses(e)[64:] == [UDPF] * 3 and rig.atk.info()["udpflood_drop"] == 131
    rig.tick(NOW + 51)                                                 # now == hold_time: released, udppps 3 > 0 though
    rig.tick(NOW + 52)                                                 # udppps 0
    _, e = rig.step(*batch([frame("udp", A, B)] * 65), now=NOW + 52)
    assert statuses(e) == [FW] * 65
    rig.close()


def test_both_sides_of_the_three_thresholds_with_ticks_between_calls(eng):
    """udp_speed, syn_speed and syn_count are strict bounds; each call is several chunks of 64."""
    td = {1: dict(drop_pack=1, flood_udp=1, udp_speed=70), 2: dict(drop_pack=1, flood_syn=1, syn_speed=70, syn_count=1 << 30),
          3: dict(drop_pack=1, flood_syn=0, syn_count=66)}
    rig = HostRig(eng, td=td, hold=50, capacity=1024)
    rig.chunk = 64
    fresh = iter(range(1, 1 << 20))

    def run(nu, ns, nc, now):
        fr = [frame("udp", A, B)] * nu + [frame("syn", A, B)] * ns + [frame("syn", A + next(fresh), B) for _ in range(nc)]
        _, e = rig.step(*batch(fr), ports=np.array([1] * nu + [2] * ns + [3] * nc, np.uint8), now=now)
        st = statuses(e)
        return set(st[:nu]), set(st[nu:nu + ns]), set(st[nu + ns:])
    fw = {FW}
    assert run(70, 70, 66, NOW) == (fw, fw, fw)
    rig.tick(NOW + 1)                                   # 70, 70, 66: each equal to its threshold
    assert [rig.m.atk.ai[1]["udppps"], rig.m.atk.ai[2]["synpps"], rig.m.atk.ai[3]["syncount"]] == [70, 70, 66]
    assert run(71, 71, 67, NOW + 1) == (fw, fw, fw)     # equal passes
    rig.tick(NOW + 2)                                   # 71, 71, 67: each one above
    rig.clock(NOW + 2)
    assert run(65, 65, 65, NOW + 2) == ({UDPF}, {SYNF}, {SYNC})
    info = rig.atk.info()
    assert (info["udpflood_drop"], info["synflood_drop"], info["syncount_drop"], info["land_drop"]) == (65, 65, 65, 0)
    assert info["ai"][1]["udp_flood_hold_time"] == NOW + 52 and info["ai"][2]["syn_flood_hold_time"] == NOW + 52
    rig.tick(NOW + 3)                                   # pps 65 but held; syncount 0: the count monitor lets go
    assert run(2, 2, 2, NOW + 3) == ({UDPF}, {SYNF}, fw)
    rig.close()


@pytest.mark.parametrize("capacity,extra", [(8, 0), (48, 20)], ids=["revoke", "checked-fits"])
def test_pool_exhaustion_inside_one_small_chunk(eng, capacity, extra):
    """40 SYN creators in one chunk of at most ACUT packets (one launch, kind 4): capacity 8, finalize's revoke path
    with ATK: only the eight granted creators count in syncount_accum, per port; capacity 48 with 20 repeats behind them,
    the overflow check runs and the exact count fits."""
    for pinned in (False, True):
        rig = HostRig(eng, capacity=capacity)
        rig.pinned = pinned
        fr = [frame("syn", A + i, B) for i in range(40)] + [frame("syn", A + i, B) for i in range(extra)]
        ports = (np.arange(40 + extra) % 4).astype(np.uint8)
        ports[5] = 4 + 1                                               # (port & 3 = 1)
        _, e = rig.step(*batch(fr), ports=ports)
        assert eng.flow_launch_info() == (4, 1)
        granted = min(capacity, 40)
        assert statuses(e)[:40] == [FW] * granted + [NOMEM] * (40 - granted)
        want = [int(((np.arange(granted) % 4) == p).sum()) for p in range(4)]
        assert [rig.atk.info()["ai"][p]["syncount_accum"] for p in range(4)] == want
        assert rig.check()["live"] == granted
        rig.step(*batch(fr), ports=ports, now=NOW + 1)                 # again: the granted flows are found
        rig.close()


@pytest.mark.parametrize("nrules,tune,image", [(64, dict(), "lds"), (4096, dict(), "split"),
                                               (64, dict(lds_image=0), "global")], ids=["lds", "split", "global"])
def test_each_image_placement(eng, nrules, tune, image):
    """The one-launch kernel with the monitors over each placement of the flow-table plan, confirmed by the planner."""
    rules = synth.make_rules(nrules, seed=31)
    old = eng.tuning()
    try:
        eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
        eng.tuning(**tune)
        img, tn, p = eng.image(), abi.Tuning(**eng.tuning()), abi.Plan()
        assert eng.lib.ppe_plan_image(img.ctypes.data, len(img), C.byref(tn), 1, C.byref(p)) == 0
        assert ("global", "lds", "split")[p.mode] == image, p.as_dict()
        rig = HostRig(eng, rules, pd=PD, td=TD, hold=1, capacity=300, commit=False)
        for k, n in enumerate((65, ACUT - 3, 5, ACUT, ACUT + 1, CUTOFF)):
            rig.pinned = bool(k & 1)
            pk = synth.make_flow_packets(n, rules, n_flows=400, seed=7300 + k, template_seed=7000, kind="udp64", stride=64,
                                         malformed_frac=0.02, syn_frac=0.5)
            ports = np.random.default_rng(k).integers(0, 4, n).astype(np.uint8)
            rig.clock(NOW + k)
            rig.step(pk["hdr"], pk["len"], ports, now=NOW + k, what=f"{image} n={n}")
            assert eng.flow_launch_info() == ((4, 1) if n <= ACUT else (0, 2))
            rig.tick(NOW + k + 1)
        assert rig.m.ft.stats()["live"] > 0 and any(rig.m.atk.totals.values())
        rig.close()
    finally:
        eng.tuning(**old)


def test_null_ports_count_on_port_zero_and_the_sticky_table_is_ignored(eng):
    rig = HostRig(eng, capacity=64)
    sticky = torch.full((130,), 3, dtype=torch.uint8, device=DEV)
    rig.atk.ports([sticky])                                            # ppe_attack_ports' table: all 3s
    fr = [frame("syn", A + i, B) for i in range(65)] + [frame("udp", A, B)] * 65
    for chunk, pinned in ((0, False), (64, False), (0, True)):
        rig.chunk, rig.pinned = chunk, pinned
        before = [accum(rig, p) for p in range(4)]
        rig.step(*batch(fr), ports=np.ones(130, np.uint8), now=NOW)    # the call's bytes: all 1s
        after = [accum(rig, p) for p in range(4)]
        assert after[3] == before[3] == (0, 0, 0) and after[0] == before[0] and after[1] != before[1]
        rig.step(*batch(fr), ports=None, now=NOW)                      # NULL: port 0
        assert accum(rig, 0) != after[0] and accum(rig, 1) == after[1] and accum(rig, 3) == (0, 0, 0)
        info = rig.atk.info()["ai"]
        assert info[3]["udp_accum"] + info[3]["syn_accum"] + info[3]["syncount_accum"] == 0
    rig.close()


@pytest.mark.parametrize("chunk", [64, 0])
def test_frozen_monitor_scenario_through_the_host_call(eng, chunk):
    """tests/golden/attack_flow_v1.npz through the new call; its ticks and aging steps run between the calls."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_attack_flow_golden as gen
    finally:
        sys.path.pop(0)
    g = np.load(GOLDEN / "attack_flow_v1.npz")
    rig = HostRig(eng, pd=gen.PD, td=gen.TD, hold=gen.HOLD, capacity=gen.CAPACITY)
    rig.chunk = chunk
    b = 0
    for step in gen.scenario():
        if step[0] == "tick":
            rig.tick(step[1])
            continue
        if step[0] == "age":
            rig.age(step[1], gen.TIMEOUT)
            continue
        _, now, kinds, ports, land, host = step
        rig.clock(now)
        rig.pinned = bool(b & 1)
        hdr, lens = batch(gen.frames_of(kinds, land, host))
        got, _ = rig.step(hdr, lens, ports, now=now, what=f"batch {b}")
        for k in ("verdict", "flow_hash", "acl_hit"):
            assert np.array_equal(got[k], g[f"{k}{b}"]), (k, b)
        assert np.array_equal(gen.table(eng.flow_dump()), g[f"table{b}"]), b
        b += 1
    assert b == int(g["nbatch"][0])
    rig.close()


# ---- the monitors and the detector together (ppe_flow_combine on) ----
class CombinedHostRig(CombinedRig):
    """test_gpu_flow_combined.Rig whose batches go through ppe_classify_flow_host_ports in chunks."""
    chunk, pinned = 0, False

    def enqueue(self, hdr, lens, ports=None, ts=None, outs=PLAIN):
        out = host_alloc(len(lens), PLAIN, self.pinned)
        rc = ports_call(self.eng, hdr, lens, ports, out, self.eng.cfg(0, self.syn_check, self.now), self.chunk,
                        self.pinned, ts=ts)
        assert rc == 0, (rc, self.eng.lib.ppe_last_error(self.eng.ctx))
        return out, self.o.cfg(0, self.syn_check, self.now)


@pytest.mark.parametrize("chunk", [64, 0])
def test_frozen_combined_scenario_through_the_host_call(eng, chunk):
    """tests/golden/flow_combined_v1.npz through the new call (kind 3 per chunk), ticks and aging between the calls."""
    g = np.load(tcm.GOLDEN)
    seq, par = tcm.gen_combined(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    rig = CombinedHostRig(eng, fpm.gen_rules(), pd=tcm.GEN_PD, td=tcm.GEN_TD, atk_hold=tcm.GEN_HOLD,
                          flow_capacity=par["flow_capacity"], ps_capacity=par["ps_capacity"], freq=par["freq"],
                          hold=par["hold"], rate=par["rate"], max_batch=1024, ps_max_batch=1024)
    rig.chunk = chunk
    try:
        at = 0
        for b, s in enumerate(seq):
            if s["tick"]:
                rig.tick(s["now_s"], check=False)
            rig.clock(s["now_c"], s["now_s"])
            rig.pinned = bool(b & 1)
            got, _ = rig.step(s["hdr"], s["lens"], s["ports"], s["ts"], what=f"batch {b}")
            n = len(s["lens"])
            for k in ("verdict", "flow_hash", "acl_hit"):
                assert np.array_equal(got[k], g[k][at:at + n]), (k, b)
            at += n
            if s["age"]:
                rig.age(s["now_s"], s["now_c"])
        assert at == len(g["verdict"])
        assert np.array_equal(np.array(table(eng.flow_dump()), np.uint64).reshape(-1, 10), g["flows"])
    finally:
        rig.close()


def combined_rig(eng, **kw):
    _, par = tcm.generated()
    return CombinedHostRig(eng, fpm.gen_rules(), pd=tcm.GEN_PD, td=tcm.GEN_TD, atk_hold=tcm.GEN_HOLD,
                           flow_capacity=par["flow_capacity"], ps_capacity=par["ps_capacity"], freq=par["freq"],
                           hold=par["hold"], rate=par["rate"], **kw)


@pytest.mark.parametrize("chunk", [64, "max", 0])
def test_combination_in_chunks_over_4133_packets(eng, chunk):
    """A warm-up call and 4,133 generated packets with the monitors and the detector both flow-attached and the switch on:
    chunks of 64, of ppe_flow_portscan_max() and of the default, each through the combined kernel, equal to the model fed
    the whole batch."""
    rig = combined_rig(eng, max_batch=8192, ps_max_batch=8192)
    rig.chunk = eng.flow_portscan_max() if chunk == "max" else chunk
    rng = np.random.default_rng(77)
    try:
        rig.clock(10_000, 1000)
        hdr, lens, ports = cbatch(rng, 700)
        rig.step(hdr, lens, ports, np.full(700, 1000, np.uint64), what="warm-up")
        rig.tick(1001)
        rig.clock(11_500, 1001)
        hdr, lens, ports = cbatch(rng, 4133)
        rig.step(hdr, lens, ports, (1001 + rng.integers(0, 3, 4133)).astype(np.uint64), what="4,133 packets")
        assert eng.flow_launch_info() == (3, 1)
        assert any(rig.m.atk.totals.values()) and rig.m.fp.ps.counts["drop"] > 0
    finally:
        rig.close()


def test_combination_with_the_switch_off_is_refused_with_nothing_touched(eng):
    rig = combined_rig(eng)
    rng = np.random.default_rng(5)
    try:
        rig.clock(10_000, 1000)
        hdr, lens, ports = cbatch(rng, 100)
        rig.step(hdr, lens, ports, what="one call first")
        eng.flow_combine(0)
        for pinned in (False, True):
            out = host_alloc(100, PLAIN, pinned)
            rc = ports_call(eng, hdr, lens, ports, out, eng.cfg(0, 1, 1000), 64, pinned)
            assert rc == abi.PPE_ENOTSUP and b"both flow-attached" in eng.lib.ppe_last_error(eng.ctx)
            assert all((v.numpy() == -7).all() for v in out.values())
            rig.same("after the refusal")
        eng.flow_combine(1)
        rig.step(hdr, lens, ports, what="and on again")
    finally:
        rig.close()


# ---- outside the monitors ----
@pytest.mark.parametrize("n", [64, 4133])
def test_nothing_attached_is_ppe_classify_flow_host(eng, n):
    """No object flow-attached: outputs, counters, table and launch kinds byte for byte ppe_classify_flow_host's; the
    port bytes are ignored."""
    rules = synth.make_rules(256, seed=21)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    pks = [synth.make_flow_packets(n, rules, n_flows=300, seed=7900 + k, template_seed=7000, kind="udp64", stride=64,
                                   malformed_frac=0.02, syn_frac=0.5) for k in range(2)]
    runs = []
    for plain in (True, False):
        eng.flow_create(200, 8192)
        eng.clear_counters()
        res = []
        try:
            for k, pk in enumerate(pks):
                for chunk, pinned in ((0, False), (128, False), (0, True)):
                    out = host_alloc(n, PLAIN, pinned)
                    rc = ports_call(eng, pk["hdr"], pk["len"], np.full(n, 3, np.uint8), out, eng.cfg(0, 1, NOW + k), chunk,
                                    pinned, plain=plain)
                    assert rc == 0
                    res.append(({x: v.numpy().tobytes() for x, v in out.items()}, eng.flow_launch_info()))
            info = eng.flow_info()
            runs.append((res, eng.counters(), table(eng.flow_dump()), (info["live"], info["new_flow"])))
        finally:
            eng.flow_destroy()
    assert runs[0] == runs[1]
    assert runs[1][0][0][1] == ((1, 1) if n <= CUTOFF else (0, 2))


def test_refusals_touch_nothing_and_the_table_stays_usable(eng):
    """Every refusal ppe_classify_flow_host has is kept (stream tracking, a stateless-attached table or object, lists or
    packed, no verdict, max_batch below one tile); ppe_classify_flow_host itself still refuses monitors flow-attached."""
    rig = HostRig(eng, pd=PD, td=TD, capacity=64)
    hdr, lens, ports = mixed(65, 1)
    rig.step(hdr, lens, ports)
    cfg = eng.cfg(0, 1, NOW)

    def state():
        cnt = eng.counters()
        return table(eng.flow_dump()), eng.flow_info()["live"], [cnt[c] for c in abi.COUNTERS], rig.atk.info()
    before = state()

    def refused(code, outs=PLAIN, pinned=False, plain=False):
        out = host_alloc(65, outs, pinned)
        rc = ports_call(eng, hdr, lens, ports, out, cfg, 64, pinned, plain=plain)
        assert rc == code, (rc, code, eng.lib.ppe_last_error(eng.ctx))
        for k, v in out.items():
            assert (v.numpy() == (0xEE if k == "part8" else -7)).all(), f"{k} written by a refused call"
        assert state() == before
    for pinned in (False, True):
        refused(abi.PPE_EINVAL, ("flow_hash", "acl_hit"), pinned)
        for extra in ("fw_idx", "drop_idx", "tile_cnt", "part8", "packed"):
            refused(abi.PPE_EINVAL, ("verdict", extra), pinned)
        eng.stream_tcp(1, 0, 0)
        refused(abi.PPE_ENOTSUP, pinned=pinned)
        eng.stream_tcp(0, 0, 0)
        ps = eng.portscan(capacity=64, max_batch=4096)
        refused(abi.PPE_ENOTSUP, pinned=pinned)
        ps.close()
        other = eng.attack()                                           # a second object, on the stateless point
        refused(abi.PPE_ENOTSUP, pinned=pinned)
        other.close()
        refused(abi.PPE_ENOTSUP, pinned=pinned, plain=True)            # ppe_classify_flow_host: monitors flow-attached
        assert b"attack monitors flow-attached" in eng.lib.ppe_last_error(eng.ctx)
    rig.step(hdr, lens, ports, now=NOW + 1, what="usable afterwards")
    # max_batch below one tile
    eng.flow_destroy()
    eng.flow_create(64, 63)
    out = host_alloc(65, PLAIN, False)
    assert ports_call(eng, hdr, lens, ports, out, cfg) == abi.PPE_EINVAL
    assert all((v.numpy() == -7).all() for v in out.values()) and eng.flow_info()["live"] == 0
    rig.close()


def test_python_wrapper(eng):
    """Engine.classify_flow_host_ports with numpy arrays (staged) and pinned tensors (in place)."""
    rig = HostRig(eng, pd=PD, td=TD, capacity=64)
    hdr, lens, ports = mixed(130, 9)
    exp = rig.m.classify_batch(hdr, lens, ports, cfg=rig.o.cfg(0, 1, NOW))
    got = eng.classify_flow_host_ports(hdr, lens, ports, cfg=eng.cfg(0, 1, NOW), chunk=64)
    compare(got, exp, 130, "numpy")
    rig.check("numpy")
    exp = rig.m.classify_batch(hdr, lens, ports, cfg=rig.o.cfg(0, 1, NOW))
    out = {k: torch.full((130, 4) if k == "tuple" else (130,), -7, dtype=torch.int32).pin_memory() for k in PLAIN}
    eng.classify_flow_host_ports(host_in(hdr, np.uint8, True), host_in(np.ascontiguousarray(lens, np.uint32), np.int32, True),
                                 host_in(ports, np.uint8, True), cfg=eng.cfg(0, 1, NOW), out=out)
    got = {k: (v.numpy() if k == "acl_hit" else v.numpy().view(np.uint32)) for k, v in out.items()}
    compare(got, exp, 130, "pinned")
    assert eng.flow_launch_info() == (4, 1)
    rig.check("pinned")
    with pytest.raises(ValueError):
        eng.classify_flow_host(hdr, lens, ports=ports)
    rig.close()

