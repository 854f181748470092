"""The attack monitors and the port-scan detector together on the flow-table path (ppe_flow_combine,
csrc/ppe_kernels_flow_portscan_attack.hip): an engine with a flow table, a port-scan table and an attack object both
flow-attached and the switch on, the serial model beside it (tests/flow_combined_model.py).  After every batch, tick and
aging step the verdict, flow hash, ACL hit, tuple and compacted lists, the 32 counters, ppe_attack_info, ppe_portscan_info
and the whole ppe_portscan_dump, ppe_flow_info and the whole ppe_flow_dump must equal the model's, the batch must have
taken one launch of kind 3, and the 64 guard entries behind every output must be untouched.  Integer work: no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import portscan_model as psm  # noqa: E402
import pyoracle  # noqa: E402
import test_flow_combined_model as tcm  # noqa: E402
import test_flow_portscan_model as tm  # noqa: E402
from attack_model import AttackModel, frame  # noqa: E402
from flow_combined_model import FlowCombinedModel  # noqa: E402
from pktbuild import udp_packet  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from test_gpu_attack import DEV, PART, PART8, PD, PLAIN, SEP, TD, alloc, collect, compare, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

LAYOUTS = (SEP, PART, PART8, PLAIN)  # (the flow path has no packed layout)
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
PS_INFO = ("live", "new_pcb", "del_pcb", "ok", "nomem", "detected", "hold", "drop")
A, B, S = tm.A, tm.B, tm.S
P24, AFW, FNOMEM = tm.P24, tm.AFW, tm.FNOMEM
LAND, SYNF, SYNC, UDPF = tcm.LAND, tcm.SYNF, tcm.SYNC, tcm.UDPF
NEWFLOW = abi.F_NEWFLOW
FLOOD_SYN0 = dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)
FLOOD_UDP0 = dict(drop_pack=1, flood_udp=1, udp_speed=0)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def MAX(eng):
    return eng.flow_portscan_max()


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "eng" in request.fixturenames:
        e = request.getfixturevalue("eng")
        for mark in ("attack_flow_attached", "attack_attached", "portscan_attached", "portscan_flow_attached"):
            if getattr(e, mark, None) is not None:
                getattr(e, mark).close()
        e.stream_tcp(0, 0, 0)
        e.flow_combine(0)


class Rig:
    """An engine with a flow table, a port-scan table and an attack object both flow-attached and ppe_flow_combine on,
    and the model: step() runs one batch through both and compares everything."""

    def __init__(self, eng, rules, default_action=DROP, pd=None, td=None, atk_hold=600, flow_capacity=100, ps_capacity=100,
                 freq=3, hold=100, action=0, rate=1000, syn_check=1, max_batch=1 << 14, ps_max_batch=2048, commit=True,
                 combine=1):
        self.eng, self.syn_check = eng, syn_check
        if commit:
            eng.commit(rules, default_action=default_action)
        eng.flow_create(flow_capacity, max_batch)
        eng.clear_counters()
        self.o = pyoracle.Oracle(rules, default_action=default_action)
        fp = fpm.FlowPortScanModel(self.o, flow_capacity, psm.PortScanModel(1, action, freq, hold, ps_capacity, rate))
        self.m = FlowCombinedModel(self.o, AttackModel(pd, td, atk_hold), fp)
        self.ps = eng.portscan(attach="flow", able=1, action=action, exception_freq=freq, hold_seconds=hold,
                               capacity=ps_capacity, max_batch=ps_max_batch, cycles_per_second=rate)
        self.atk = eng.attack(self.m.atk.cfg(), attach="flow")
        eng.flow_combine(combine)
        self.counters = np.zeros(32, np.uint64)
        self.now = 0
        self.keep = []  # (the port arrays of the queued batches stay alive)

    def close(self):
        self.atk.close()
        self.ps.close()
        self.eng.flow_destroy()
        self.eng.flow_combine(0)

    def clock(self, cycles, seconds):
        self.ps.clock(cycles, seconds)
        self.m.fp.ps.clock(cycles, seconds)
        self.atk.clock(seconds)
        self.m.atk.clock(seconds)
        self.now = seconds

    def tick(self, seconds, check=True):
        self.atk.tick(seconds)
        self.m.atk.tick(seconds)
        if check:
            self.same("after a tick")

    def able(self, v):
        self.ps.set(able=v)
        self.m.fp.ps.able = v

    def enqueue(self, hdr, lens, ports=None, ts=None, outs=SEP):
        th, tl, tp = to_dev(hdr, lens, ports)
        self.atk.ports([tp] if tp is not None else None)
        tts = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV) if ts is not None else None
        out = alloc(len(lens), outs)
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, self.syn_check, self.now), ts=tts)
        self.keep.append((th, tl, tp, tts))
        return out, self.o.cfg(0, self.syn_check, self.now)

    def check(self, out, hdr, lens, ports, ts, cfg, what=""):
        n = len(lens)
        ref = self.m.classify_batch(hdr, lens, ports, ts, cfg)
        got = collect(out, n)
        compare(got, ref, n, what)
        self.counters += ref["counters"]
        return got, ref

    def step(self, hdr, lens, ports=None, ts=None, outs=SEP, what=""):
        out, cfg = self.enqueue(hdr, lens, ports, ts, outs)
        torch.cuda.synchronize()
        got, ref = self.check(out, hdr, lens, ports, ts, cfg, what)
        assert self.eng.flow_launch_info() == ((3, 1) if self.m.fp.ps.able == 1 else (0, 2)), what
        self.same(what)
        return got, ref

    def same(self, what=""):
        cnt = self.eng.counters()
        assert [cnt[c] for c in abi.COUNTERS] == self.counters[:len(abi.COUNTERS)].tolist(), what
        assert table(self.eng.flow_dump()) == self.m.table(), what
        info, st = self.eng.flow_info(), self.m.stats()
        assert (info["live"], info["new_flow"], info["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        pi, mi = self.ps.info(), self.m.fp.ps.info()
        assert {k: pi[k] for k in PS_INFO} == {k: mi[k] for k in PS_INFO}, what
        assert fpm.ps_records(self.ps.dump()) == self.m.fp.ps.records(), what
        ai, want = self.atk.info(), self.m.info()
        for p in range(4):
            g = {k: ai["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
            assert g == want["ai"][p], (what, "port", p, g, want["ai"][p])
        assert {k: ai[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}, what
        return info

    def age(self, now_s, now_c, timeout=2):
        assert self.eng.flow_age(now_s, timeout) == self.m.age(now_s, timeout)
        assert self.ps.age(now_c) == self.m.fp.ps.timeout(now_c)
        self.same("after aging")


def statuses(r):
    return (r["verdict"] & 0xFF).tolist()


def is_new(r, i):
    return bool((int(r["verdict"][i]) >> 16) & NEWFLOW)


def cbatch(rng, n):
    """fpm.gen_batch's population with a port byte per packet and some SYNs made land packets on port 0."""
    hdr, lens = fpm.gen_batch(rng, n)
    ports = rng.integers(0, 4, n).astype(np.uint8)
    for i in np.flatnonzero(rng.random(n) < 0.08):
        if hdr[i, 23] == 6 and hdr[i, 47] & 0x02:
            hdr[i, 30:34] = hdr[i, 26:30]
            ports[i] = 0
    return hdr, lens, ports


def gen_rig(eng, par, **kw):
    return Rig(eng, fpm.gen_rules(), pd=tcm.GEN_PD, td=tcm.GEN_TD, atk_hold=tcm.GEN_HOLD, flow_capacity=par["flow_capacity"],
               ps_capacity=par["ps_capacity"], freq=par["freq"], hold=par["hold"], rate=par["rate"], **kw)


@pytest.mark.parametrize("name", sorted(tcm.KATS))
def test_known_answers(eng, name):
    """tests/test_flow_combined_model.py's hand-derived answers a-i, against the stated answers and the model."""
    k = tcm.KATS[name]
    rig = Rig(eng, tm.kat_rules(), pd=k.get("pd"), td=k.get("td"), flow_capacity=k.get("flow_capacity", 100),
              ps_capacity=k.get("ps_capacity", 100))
    try:
        for j, step in enumerate(k["steps"]):
            if "tick" in step:
                rig.tick(step["tick"])
            rig.clock(*step["clock"])
            hdr, lens = tm.stack(step["frames"])
            ts = np.array(step["ts"], np.uint64) if "ts" in step else None
            ports = np.array(step["ports"], np.uint8) if "ports" in step else None
            got, ref = rig.step(hdr, lens, ports, ts, outs=LAYOUTS[j % 4], what=f"{name} step {j}")
            tm.check_step(step, got, (name, j))
            assert ref["results"].tolist() == [-1 if r is None else r for _, _, r in step["want"]]
            ai = rig.atk.info()
            tcm.check_kat_state(step, tcm.accums(ai["ai"]), ai, eng.flow_info()["live"], fpm.ps_records(rig.ps.dump()),
                                rig.ps.info(), table(eng.flow_dump()), (name, j))
        if name == "h_all_dropped":  # no packet was pending: no resolve round, no tombstone
            assert eng.flow_portscan_rounds() == 0 and eng.flow_info()["tombstones"] == 0
    finally:
        rig.close()


def test_sizes_and_the_refusal_above_the_maximum(eng, MAX):
    """n in {1, 63, 64, 65, MAX - 1, MAX} on one set of tables with a tick between the batches; MAX + 1 is refused with
    nothing written and all three states unchanged."""
    _, par = tcm.generated()
    rig = gen_rig(eng, par)
    rng = np.random.default_rng(11)
    try:
        for k, n in enumerate((1, 63, 64, 65, MAX - 1, MAX, 65, 1)):
            rig.tick(1000 + k)
            rig.clock(10_000 + 400 * k, 1000 + k)
            hdr, lens, ports = cbatch(rng, n)
            rig.step(hdr, lens, ports, (1000 + k + rng.integers(0, 3, n)).astype(np.uint64), outs=LAYOUTS[k % 4],
                     what=f"n={n}")
        assert any(rig.m.atk.totals.values()) and rig.m.fp.ps.counts["drop"] > 0
        hdr, lens, ports = cbatch(rng, MAX + 1)
        th, tl, tp = to_dev(hdr, lens, ports)
        rig.atk.ports([tp])
        out = alloc(MAX + 1, SEP)
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 2000))
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v.cpu().numpy() == -7).all(), k
        rig.same("after the refusal")
        rig.able(0)  # the detector off: the same batch through the kernels with the monitors alone
        rig.step(hdr, lens, ports, what="able 0 above the maximum")
    finally:
        rig.close()


def held_rig(eng, sources, **kw):
    """Every source of `sources` held until ts 601 (tm.prime / tm.hot: five UDP packets each, on port 0)."""
    rig = Rig(eng, tm.kat_rules(), **kw)
    rig.clock(10000, 500)
    rig.step(*tm.stack([f for s in sources for f in tm.prime(s)["frames"]]), what="prime")
    rig.clock(11500, 501)
    got, _ = rig.step(*tm.stack([f for s in sources for f in tm.hot(s)["frames"]]), what="hot")
    assert statuses(got) == [P24] * len(sources)
    return rig


def test_creator_and_its_dropped_lower_claimer_across_the_tile_boundary(eng):
    """A held until ts 601: its SYNs of tuples W and Y at ts 600 (indices 63 and 5, port 1) claim their slots and are
    dropped by the detector (HOLD); the same SYNs at ts 601 (indices 64 and 70, port 2) create the flows: a creator in
    tile 1 whose dropped lower claimer is the last lane of tile 0, and one whose lower claimer lies deep in tile 0.  B the
    same inside tile 0 (dropped at 10, creator at 20), and C with the creator in tile 0 and a later SYN of the tuple in
    tile 1 dropped by a monitor (SYN flood held on port 3), which never reaches the table.  syncount_accum counts the
    four creators on their own ports."""
    c3 = 0x0A000003
    rig = held_rig(eng, (A, B), td={3: FLOOD_SYN0})
    try:
        rig.step(*tm.stack([tm.syn(0x0A000009, 1, sp=9)]), ports=np.array([3], np.uint8), what="arm port 3")
        rig.tick(502)                                     # port 3: synpps 1 > 0
        n = 130
        fr = [frame("icmp", 0x0A000100 + i, S) for i in range(n)]
        ports, ts = np.zeros(n, np.uint8), np.full(n, 600, np.uint64)
        place = {"Y": (A, 40001, 5, 70), "W": (A, 40002, 63, 64), "V": (B, 40003, 10, 20)}   # (dropped, creator)
        for src, cp, drp, cre in place.values():
            fr[drp] = fr[cre] = tm.syn(src, cp)
            ports[drp], ports[cre], ts[cre] = 1, 2, 601
        fr[62] = fr[65] = tm.syn(c3, 40004)               # C: creator in tile 0, the monitor-dropped SYN in tile 1
        ports[62], ports[65] = 2, 3
        rig.clock(14500, 502)
        got, ref = rig.step(*tm.stack(fr), ports=ports, ts=ts, outs=SEP, what="across the boundary")
        st = statuses(got)
        for _, _, drp, cre in place.values():
            assert st[drp] == P24 and st[cre] == AFW and is_new(got, cre), (drp, cre)
        assert st[62] == AFW and is_new(got, 62) and st[65] == SYNF
        acc = tcm.accums(rig.atk.info()["ai"])
        assert acc[1] == (0, 3, 0) and acc[2] == (0, 4, 4) and acc[3][2] == 0
        assert eng.flow_info()["live"] == 4
        # the other order: the creators' SYNs again, now found; a dropped SYN's tuple alone leaves no flow
        rig.step(*tm.stack(fr[::-1]), ports=ports[::-1].copy(), ts=np.full(n, 601, np.uint64), outs=PART,
                 what="reversed")
    finally:
        rig.close()


def test_one_source_chain_interleaved_with_its_monitor_dropped_syns(eng):
    """One source's SYNs of nine new tuples at indices 60-68; those at 62, 64 and 66 arrive on port 0, whose SYN flood is
    held: they leave the classify phase final and are no part of the source's chain, which runs 60, 61, 63, 65, 67, 68
    in six rounds without waiting on them."""
    rig = Rig(eng, tm.kat_rules(), td={0: FLOOD_SYN0})
    try:
        rig.clock(10000, 500)
        rig.step(*tm.stack([tm.syn(B, 1, sp=9)]), ports=np.zeros(1, np.uint8), what="arm port 0")
        rig.tick(501)
        n = 130
        fr = [frame("icmp", 0x0A000100 + i, S) for i in range(n)]
        ports = np.ones(n, np.uint8)
        for i in range(60, 69):
            fr[i] = tm.syn(A, 41000 + i)
        ports[[62, 64, 66]] = 0
        rig.clock(10200, 501)
        got, ref = rig.step(*tm.stack(fr), ports=ports, outs=PART8, what="chain")
        st = statuses(got)
        assert [st[i] for i in (62, 64, 66)] == [SYNF] * 3
        assert all(st[i] == AFW and is_new(got, i) for i in (60, 61, 63, 65, 67, 68))
        assert ref["results"][60:69].tolist() == [psm.OK, psm.OK, -1, psm.OK, -1, psm.OK, -1, psm.OK, psm.OK]
        assert eng.flow_portscan_rounds() == 6
        assert tcm.accums(rig.atk.info()["ai"])[:2] == [(0, 3, 0), (0, 6, 6)]
        # a batch wholly monitor-dropped behind it: the round count reads 0, neither table moves
        before = (table(eng.flow_dump()), fpm.ps_records(rig.ps.dump()), eng.flow_info()["tombstones"])
        got, _ = rig.step(*tm.stack([tm.syn(A + i, 42000) for i in range(n)]), ports=np.zeros(n, np.uint8), outs=SEP,
                          what="all dropped")
        assert statuses(got) == [SYNF] * n and eng.flow_portscan_rounds() == 0
        assert (table(eng.flow_dump()), fpm.ps_records(rig.ps.dump()), eng.flow_info()["tombstones"]) == before
    finally:
        rig.close()


def test_thresholds_across_ticks_without_a_synchronise(eng):
    """Both sides of udp_speed, syn_speed and syn_count (strict >): three batches with a tick enqueued between them and
    no synchronise until the end.  The statuses are worked out by hand (as tests/test_gpu_attack_flow.py's)."""
    td = {1: dict(drop_pack=1, flood_udp=1, udp_speed=7), 2: dict(drop_pack=1, flood_syn=1, syn_speed=7, syn_count=1 << 30),
          3: dict(drop_pack=1, flood_syn=0, syn_count=5)}
    rig = Rig(eng, np.zeros(0, abi.RULE_DTYPE), default_action=FW, td=td, atk_hold=50, flow_capacity=256)
    fresh = iter(range(1, 1 << 20))
    try:
        rig.clock(10000, 500)
        queued = []

        def enqueue(nu, ns, nc):
            """nu UDP on port 1, ns SYNs of one flow on port 2, nc SYNs of new flows on port 3."""
            fr = [udp_packet(A, S, 5000, 80)] * nu + [tm.syn(A, 40000)] * ns + \
                 [tm.syn(0x0A000100 + next(fresh), 40000) for _ in range(nc)]
            hdr, lens = tm.stack(fr)
            ports = np.array([1] * nu + [2] * ns + [3] * nc, np.uint8)
            out, cfg = rig.enqueue(hdr, lens, ports, outs=LAYOUTS[len(queued) % 4])
            ref = rig.m.classify_batch(hdr, lens, ports, None, cfg)   # (the model runs in stream order, as the ticks do)
            rig.counters += ref["counters"]
            queued.append((out, ref, (nu, ns, nc)))
        enqueue(7, 7, 5)
        rig.tick(501, check=False)     # udppps 7, synpps 7, syncount 5: each equal to its threshold
        enqueue(8, 8, 6)               # equal passes
        rig.tick(502, check=False)     # 8, 8, 6: each one above
        enqueue(3, 3, 3)
        torch.cuda.synchronize()
        assert eng.flow_launch_info() == (3, 1)
        want = [({AFW}, {AFW}, {AFW}), ({AFW}, {AFW}, {AFW}), ({UDPF}, {SYNF}, {SYNC})]
        for k, (out, ref, (nu, ns, nc)) in enumerate(queued):
            got = collect(out, nu + ns + nc)
            compare(got, ref, nu + ns + nc, f"batch {k}")
            st = statuses(got)
            assert (set(st[:nu]), set(st[nu:nu + ns]), set(st[nu + ns:])) == want[k], k
        rig.same("at the end")
        info = rig.atk.info()
        assert (info["udpflood_drop"], info["synflood_drop"], info["syncount_drop"], info["land_drop"]) == (3, 3, 3, 0)
    finally:
        rig.close()


def test_max_sources_against_three_records(eng, MAX):
    """MAX sources, one UDP packet each; port 1's UDP flood is held, so its packets are no candidates: the arming packet's
    source holds one of the three records, the first two survivors take the others, every later survivor is NOMEM."""
    rig = Rig(eng, np.zeros(0, abi.RULE_DTYPE), default_action=FW, td={1: FLOOD_UDP0}, flow_capacity=4096, ps_capacity=3)
    try:
        rig.clock(10_000, 500)
        rig.step(*tm.stack([udp_packet(S, A, 1, 2)]), ports=np.ones(1, np.uint8), what="arm port 1")
        rig.tick(501)
        rig.clock(10_500, 501)
        frames = [udp_packet(0x0A000001 + i, 0x0B000001, 5000, 53) for i in range(MAX)]
        ports = (np.arange(MAX) % 4).astype(np.uint8)
        got, ref = rig.step(*tm.stack(frames), ports=ports, what="MAX sources")
        surv = np.flatnonzero(ports != 1)
        assert ref["results"][surv].tolist() == [psm.OK] * 2 + [psm.NOMEM] * (len(surv) - 2)
        assert (ref["results"][ports == 1] == -1).all() and set(np.array(statuses(got))[ports == 1]) == {UDPF}
        assert rig.ps.info()["live"] == 3 and eng.flow_info()["live"] == 3
        rig.step(*tm.stack(frames[::-1]), ports=ports[::-1].copy(), outs=PART, what="again, reversed")
    finally:
        rig.close()


def test_flow_capacity_eight_with_creators_past_it(eng):
    """40 SYNs of new flows, ports cycling 0-3, port 3's SYN flood held: the thirty survivors are creators; the arming
    packet's flow holds one of the eight places, the first seven survivors in packet order get the others (indices 0, 1,
    2, 4, 5, 6, 8: ports 0, 1, 2, 0, 1, 2, 0), the rest are FLOW_NOMEM with their detector records stepped;
    syncount_accum counts the seven."""
    rig = Rig(eng, np.zeros(0, abi.RULE_DTYPE), default_action=FW, td={3: FLOOD_SYN0}, flow_capacity=8)
    try:
        rig.clock(10_000, 500)
        rig.step(*tm.stack([tm.syn(B, 1)]), ports=np.full(1, 3, np.uint8), what="arm port 3")
        rig.tick(501)
        rig.clock(10_100, 501)
        fr = [tm.syn(0x0A000100 + i, 40000) for i in range(40)]
        ports = (np.arange(40) % 4).astype(np.uint8)
        got, ref = rig.step(*tm.stack(fr), ports=ports, what="creators past the pool")
        st = statuses(got)
        surv = [i for i in range(40) if i % 4 != 3]
        assert [st[i] for i in surv] == [AFW] * 7 + [FNOMEM] * 23 and all(st[i] == SYNF for i in range(3, 40, 4))
        assert (ref["results"][surv] == psm.OK).all()
        assert [a[2] for a in tcm.accums(rig.atk.info()["ai"])] == [3, 2, 2, 0]
        assert eng.flow_info()["live"] == 8 and rig.ps.info()["live"] == 31
        rig.step(*tm.stack(fr), ports=ports, outs=PART8, what="again: the granted flows are found")
    finally:
        rig.close()


def test_sixty_generated_batches(eng, MAX):
    """tests/test_flow_combined_model.py's generated sequence (each of the cases a-g at least 10 times, by
    test_generated_sequence_holds_every_case): sizes 1..130, ticks, both tables aged in between, and a flow rehash
    brought about by the tombstones of the aging and of creator-less claims."""
    seq, par = tcm.generated()
    rig = gen_rig(eng, par, max_batch=tcm.MAX_N, ps_max_batch=tcm.MAX_N)
    try:
        for b, s in enumerate(seq):
            if s["tick"]:
                rig.tick(s["now_s"], check=False)
            rig.clock(s["now_c"], s["now_s"])
            rig.step(s["hdr"], s["lens"], s["ports"], s["ts"], outs=LAYOUTS[b % 4], what=f"batch {b}")
            if s["age"]:
                rig.age(s["now_s"], s["now_c"])
        assert eng.flow_info()["rehashes"] >= 1
    finally:
        rig.close()


@pytest.mark.parametrize("nrules,tune,image", [(64, dict(), "lds"), (4096, dict(), "split"),
                                               (64, dict(lds_image=0), "global")], ids=["lds", "split", "global"])
def test_each_image_placement(eng, MAX, nrules, tune, image):
    rules = synth.make_rules(nrules, seed=31)
    old = eng.tuning()
    try:
        eng.commit(rules, default_action=FW)
        eng.tuning(**tune)
        img, tn, p = eng.image(), abi.Tuning(**eng.tuning()), abi.Plan()
        assert eng.lib.ppe_plan_image(img.ctypes.data, len(img), C.byref(tn), 1, C.byref(p)) == 0
        assert ("global", "lds", "split")[p.mode] == image, p.as_dict()
        rig = Rig(eng, rules, default_action=FW, pd=PD, td=TD, atk_hold=1, flow_capacity=300, ps_capacity=40, freq=2,
                  hold=3, commit=False)
        try:
            for k, n in enumerate((65, MAX - 3, 5, MAX)):
                pk = synth.make_flow_packets(n, rules, n_flows=400, seed=7300 + k, template_seed=7000, kind="udp64",
                                             stride=64, malformed_frac=0.02, syn_frac=0.5)
                ports = np.random.default_rng(k).integers(0, 4, n).astype(np.uint8)
                rig.clock(10_000 + 700 * k, 1000 + k)
                rig.step(pk["hdr"], pk["len"], ports, outs=LAYOUTS[k % 4], what=f"{image} n={n}")
                rig.tick(1001 + k)
            assert rig.m.fp.ps.counts["drop"] > 0 and rig.m.stats()["live"] > 0 and any(rig.m.atk.totals.values())
        finally:
            rig.close()
    finally:
        eng.tuning(**old)


def test_frozen_scenario(eng):
    """tests/golden/flow_combined_v1.npz (ticks and aging between the batches) on the GPU."""
    g = np.load(tcm.GOLDEN)
    seq, par = tcm.gen_combined(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    rig = gen_rig(eng, par, max_batch=int(g["max_n"]), ps_max_batch=int(g["max_n"]))
    try:
        at = 0
        for b, s in enumerate(seq):
            if s["tick"]:
                rig.tick(s["now_s"], check=False)
            rig.clock(s["now_c"], s["now_s"])
            got, _ = rig.step(s["hdr"], s["lens"], s["ports"], s["ts"], outs=LAYOUTS[b % 4], what=f"batch {b}")
            n = len(s["lens"])
            for k in ("verdict", "flow_hash", "acl_hit"):
                assert np.array_equal(got[k], g[k][at:at + n]), (k, b)
            at += n
            if s["age"]:
                rig.age(s["now_s"], s["now_c"])
        assert at == len(g["verdict"])
        assert np.array_equal(np.array(table(eng.flow_dump()), np.uint64).reshape(-1, 10), g["flows"])
        assert np.array_equal(np.array(sorted(fpm.ps_records(rig.ps.dump())), np.uint64).reshape(-1, 7), g["records"])
    finally:
        rig.close()


# ---- the switch ----
def test_switch_off_refuses_and_toggles_between_batches(eng):
    """A new context has the switch at 0: both attached and able 1 is refused (-95) with nothing touched, as before the
    switch existed.  Turned on, off and on again between batches on one set of tables; values above 1 are PPE_EINVAL and
    leave it; ppe_flow_destroy leaves it too."""
    _, par = tcm.generated()
    rig = gen_rig(eng, par, combine=0)
    rng = np.random.default_rng(5)
    try:
        def refused(n):
            hdr, lens, ports = cbatch(rng, n)
            th, tl, tp = to_dev(hdr, lens, ports)
            rig.atk.ports([tp])
            out = alloc(n, SEP)
            with pytest.raises(PPEError, match="-95.*both flow-attached"):
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 1000))
            torch.cuda.synchronize()
            for k, v in out.items():
                assert (v.cpu().numpy() == -7).all(), k
            rig.same("after the refusal")
        rig.clock(10_000, 1000)
        refused(64)
        for k, on in enumerate((1, 0, 1, 1, 0, 1)):
            eng.flow_combine(on)
            rig.clock(10_000 + 500 * k, 1000 + k)
            if on:
                hdr, lens, ports = cbatch(rng, (100, 64, 300, 1)[k % 4])
                rig.step(hdr, lens, ports, outs=LAYOUTS[k % 4], what=f"toggle {k}")
                rig.tick(1001 + k)
            else:
                refused(65)
        assert eng.lib.ppe_flow_combine(eng.ctx, 2) == abi.PPE_EINVAL
        hdr, lens, ports = cbatch(rng, 10)
        rig.step(hdr, lens, ports, what="still on")
        # able 0 / 1 with the switch on: the monitors' two launches and the combined kernel alternate on one table
        for k, able in enumerate((0, 1, 0)):
            rig.able(able)
            hdr, lens, ports = cbatch(rng, 200)
            rig.step(hdr, lens, ports, outs=LAYOUTS[k % 4], what=f"able {able}")
        rig.able(1)
        eng.flow_destroy()              # the switch is the context's, like the attachments
        eng.flow_create(64, 1024)
        out = alloc(1, PLAIN)
        th, tl, _ = to_dev(*tm.stack([udp_packet()]))
        rig.atk.ports(None)
        eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 2000))
        torch.cuda.synchronize()
        assert eng.flow_launch_info() == (3, 1)
    finally:
        rig.close()


@pytest.mark.parametrize("n", [64, 8000])
@pytest.mark.parametrize("mode", ["table_only", "monitors_only", "both_able0"])
def test_switch_on_changes_nothing_outside_the_combination(n, mode):
    """Switch 1 with only the table attached, only the monitors attached, or both with able 0: byte-identical outputs,
    counters, tables and launch kinds to a twin context that never called ppe_flow_combine."""
    rules = synth.make_rules(256, seed=21)
    m = abi.load().ppe_flow_portscan_max()
    pks = [synth.make_flow_packets(n, rules, n_flows=300, seed=7900 + k, template_seed=7000, kind="udp64", stride=64,
                                   malformed_frac=0.02, syn_frac=0.5) for k in range(2)]
    ports = (np.arange(n) % 4).astype(np.uint8)
    runs = []
    for combine in (None, 1):
        e = Engine(0)
        try:
            e.commit(rules, default_action=FW)
            e.flow_create(1000, 1 << 14)
            if combine is not None:
                e.flow_combine(combine)
            ps = atk = None
            if mode != "monitors_only":
                ps = e.portscan(attach="flow", able=0 if mode == "both_able0" else 1, exception_freq=1, capacity=4,
                                max_batch=1 << 14)
            if mode != "table_only":
                atk = e.attack(AttackModel(PD, TD, 5).cfg(), attach="flow")
            res, kinds = [], []
            for k, pk in enumerate(pks):
                th, tl, tp = to_dev(pk["hdr"], pk["len"], ports)   # (table only, n > MAX: refused on both sides)
                if atk is not None:
                    atk.clock(1000 + k)
                    atk.ports([tp])
                out = alloc(n, SEP)
                try:
                    e.classify_flow_torch(th, tl, out, cfg=e.cfg(0, 1, 1000 + k))
                    rc = 0
                except PPEError as err:
                    rc = str(err)
                torch.cuda.synchronize()
                res.append((rc, {k2: v.cpu().numpy().tobytes() for k2, v in out.items()}))
                kinds.append(e.flow_launch_info())
                if atk is not None:
                    atk.tick(1001 + k)
            state = (e.counters(), table(e.flow_dump()), ps.info() if ps else None, atk.info() if atk else None)
            runs.append((res, kinds, state))
            for h in (atk, ps):
                if h is not None:
                    h.close()
        finally:
            e.close()
    assert runs[0] == runs[1]
    want = {"table_only": (2, 1) if n <= m else (0, 0), "monitors_only": (0, 2), "both_able0": (0, 2)}[mode]
    assert runs[1][1] == [want] * 2
    if mode == "table_only" and n > m:
        assert all("-95" in r[0] for r in runs[1][0])
    else:
        assert all(r[0] == 0 for r in runs[1][0])


def test_host_and_steered_paths_still_refuse(eng):
    """ppe_classify_flow_host and the steered multi-GPU path (one rank) refuse with monitors flow-attached, switch on or
    off, before anything is touched."""
    _, par = tcm.generated()
    rig = gen_rig(eng, par)
    try:
        hdr, lens, ports = cbatch(np.random.default_rng(3), 64)
        rig.clock(10_000, 1000)
        rig.step(hdr, lens, ports, what="one batch first")
        before = (rig.atk.info(), rig.ps.info())
        for on in (1, 0):
            eng.flow_combine(on)
            with pytest.raises(PPEError, match="-95"):
                eng.classify_flow_host(hdr, lens, cfg=eng.cfg(0, 1, 1000))
            from ppe.dist import DeviceSteerOps, steered_classify_flow
            th, tl, _ = to_dev(hdr, lens)
            with pytest.raises(PPEError, match="-95"):
                steered_classify_flow(DeviceSteerOps(eng), None, th, tl, eng.cfg(0, 1, 1000), 1, 0)
            torch.cuda.synchronize()
            assert (rig.atk.info(), rig.ps.info()) == before
            rig.same(f"switch {on}")
    finally:
        rig.close()
