"""The land, SYN-flood and UDP-flood monitors on the flow-table path (ppe_flow_attack_attach) on the GPU, exact against
the tests' model (tests/attack_flow_model.py: tests/attack_model.py's serial monitors ahead of pyoracle.OracleFlow,
pinned by tests/test_attack_flow.py): after every batch, tick and aging step the verdict word, ACL hit, flow hash and
tuple, every list layout the flow path writes, all 32 counters, ppe_attack_info (four ports' ten state fields, the
four drop totals), ppe_flow_info and the whole dumped table.  Every output buffer carries 64 guard entries behind its
last one, which must stay untouched.

Integer work: no tolerance anywhere."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import decode_corpus as dc  # noqa: E402
import pyoracle  # noqa: E402
from attack_flow_model import AttackFlowModel  # noqa: E402
from attack_model import AttackModel, batch, frame  # noqa: E402
from pktbuild import eth, ipv4, tcp  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_attack import PART, PART8, PD, PLAIN, SEP, TD, alloc, collect, compare, mixed, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
GOLDEN = Path(__file__).resolve().parent / "golden"
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
FW, NOMEM, NOSYN, ADROP = ST["ACL_FW"], ST["FLOW_NOMEM"], ST["FLOW_TCP_NO_SYN_FIRST"], ST["ACL_DROP"]
A, B = 0x0A000001, 0x0B000002
LAYOUTS = (SEP, PART, PART8, PLAIN)        # (the flow path has no packed layout)
FLOOD0 = dict(drop_pack=1, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=1 << 30)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "eng" in request.fixturenames:
        e = request.getfixturevalue("eng")
        for mark in ("attack_flow_attached", "attack_attached", "portscan_attached"):
            if getattr(e, mark, None) is not None:
                getattr(e, mark).close()
        e.stream_tcp(0, 0, 0)


class FlowRig:
    """An engine with a flow table and the monitors flow-attached, the model beside it: step() runs one batch through
    both and compares everything."""

    def __init__(self, eng, rules=None, default_action=abi.ACL_RULE_ACTION_FW, pd=None, td=None, hold=600,
                 capacity=4096, max_batch=8192, syn_check=1, commit=True, attach=True):
        self.eng, self.syn_check = eng, syn_check
        self.rules = np.zeros(0, abi.RULE_DTYPE) if rules is None else rules
        if commit:
            eng.commit(self.rules, default_action=default_action)
        eng.flow_create(capacity, max_batch)
        self.o = pyoracle.Oracle(self.rules, default_action=default_action)
        self.m = AttackFlowModel(self.o, capacity, AttackModel(pd, td, hold))
        self.atk = eng.attack(self.m.atk.cfg(), attach="flow" if attach else False)
        self.clock(NOW)

    def close(self):
        self.atk.close()
        self.eng.flow_destroy()
        self.m.close()

    def clock(self, now):
        self.atk.clock(now)
        self.m.atk.clock(now)

    def tick(self, now):
        self.atk.tick(now)
        self.m.atk.tick(now)
        self.check("after a tick")

    def set(self, pd=None, td=None, hold=600):
        self.m.atk.set(pd, td, hold)
        self.atk.set(self.m.atk.cfg())

    def age(self, now, timeout=20):
        assert self.eng.flow_age(now, timeout) == self.m.age(now, timeout)
        self.check("after aging")

    def classify(self, hdr, lens, ports, outs, now, syn_check):
        n = len(lens)
        th, tl, tp = to_dev(hdr, lens, ports)
        self.atk.ports([tp] if tp is not None else None)
        out = alloc(n, outs)
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, syn_check, now))
        torch.cuda.synchronize()
        return collect(out, n)

    def step(self, hdr, lens, ports=None, now=NOW, outs=SEP, syn_check=None, what="", exp=None, wide=None, punt=None,
             narrow_tuple=None, tmask=None):
        """exp: the model's answer when the caller has it already (the model is then not run).  wide / punt /
        narrow_tuple / tmask: a window narrower than the frames (tests/decode_corpus.py): the model reads the 256-B
        rows `wide`, the engine punts `punt`, and the tuple is the stateless oracle's on the narrow window."""
        n = len(lens)
        sc = self.syn_check if syn_check is None else syn_check
        self.eng.clear_counters()
        if exp is None:
            exp = self.m.classify_batch(hdr if wide is None else wide, lens, ports, cfg=self.o.cfg(0, sc, now), punt=punt)
        if narrow_tuple is not None:
            t = narrow_tuple.copy()
            t[exp["dropped"], 2] = 0
            t[exp["dropped"], 3] &= 0x1FF
            exp = dict(exp, tuple=t & tmask)
        got = self.classify(hdr, lens, ports, outs, now, sc)
        compare(got, exp, n, what, tmask)
        cnt = self.eng.counters()
        assert [cnt[c] for c in abi.COUNTERS] == exp["counters"].tolist(), (what, cnt)
        self.check(what)
        return got, exp

    def check(self, what=""):
        info, want = self.atk.info(), self.m.info()
        for p in range(4):
            g = {k: info["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
            assert g == want["ai"][p], (what, "port", p, g, want["ai"][p])
        assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}, what
        assert table(self.eng.flow_dump()) == table(self.m.ft.dump()), what
        fi, st = self.eng.flow_info(), self.m.ft.stats()
        assert (fi["live"], fi["new_flow"], fi["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        return fi


def statuses(exp):
    return (exp["verdict"] & 0xFF).tolist()


def accum(rig, port=0):
    a = rig.m.atk.ai[port]
    return a["udp_accum"], a["syn_accum"], a["syncount_accum"]


def test_known_answers(eng):
    """The CPU known answers 1-9 (tests/test_attack_flow.py) through the engine, batch by batch; the statuses asserted
    here are the hand-derived ones, everything else is compared with the model by step()."""
    syn, ack, udp = frame("syn", A, B), frame("ack", A, B), frame("udp", A, B)
    # 1, 2: two SYNs of one 5-tuple count one creation; a SYN on a live flow counts in syn_accum only
    rig = FlowRig(eng, capacity=16)
    _, e = rig.step(*batch([syn, syn]))
    assert statuses(e) == [FW, FW] and accum(rig) == (0, 2, 1)
    _, e = rig.step(*batch([syn]), now=NOW + 1, outs=PART)
    assert statuses(e) == [FW] and accum(rig) == (0, 3, 1)
    rig.close()
    # 3: capacity 1, the second creator is refused and not counted
    rig = FlowRig(eng, capacity=1)
    _, e = rig.step(*batch([syn, frame("syn", A + 1, B)]), outs=PART8)
    assert statuses(e) == [FW, NOMEM] and accum(rig) == (0, 2, 1)
    rig.close()
    # 4: syn_check 0, an ACK-only and a UDP creation do not count, a SYN creation does
    rig = FlowRig(eng, capacity=16, syn_check=0)
    _, e = rig.step(*batch([ack, frame("udp", A + 1, B), frame("syn", A + 2, B)]))
    assert statuses(e) == [FW] * 3 and all((v >> 16) & abi.F_NEWFLOW for v in e["verdict"].tolist())
    assert accum(rig) == (1, 1, 1)
    rig.close()
    # 5: a SYN the ACL drops: no flow, not counted
    rig = FlowRig(eng, capacity=16, default_action=abi.ACL_RULE_ACTION_DROP)
    _, e = rig.step(*batch([syn]))
    assert statuses(e) == [ADROP] and accum(rig) == (0, 1, 0) and rig.check()["live"] == 0
    rig.close()
    # 6, 9: SYN-flood, land and UDP-flood drops on live flows leave the flows untouched
    land = frame("syn", A, A)
    rig = FlowRig(eng, capacity=16, td={0: FLOOD0})
    _, e = rig.step(*batch([syn, land, udp, udp]))
    assert statuses(e) == [FW] * 4
    before = table(eng.flow_dump())
    rig.tick(NOW + 1)
    rig.set({0: dict(drop_pack=1, land=1)}, {0: FLOOD0})
    _, e = rig.step(*batch([syn, land, udp, frame("udp_short", A, B), ack]), now=NOW + 5)
    assert statuses(e) == [SYNF, LAND, UDPF, UDPF, FW]
    after = table(eng.flow_dump())
    assert [r for r in after if r[4] == 17] == [r for r in before if r[4] == 17]          # the UDP flow
    assert [r for r in after if r[0] == r[1]] == [r for r in before if r[0] == r[1]]      # the land flow
    assert [r for r in after if r[4] == 6 and r[0] != r[1]][0][5] == 2                    # SYN then ACK, not the drop
    rig.close()
    # 7: a land-dropped SYN creates no flow: the reverse-direction packet behind it is a miss
    l4 = tcp(80, 1234, 0x10, payload=b"\0" * 6)
    rev = eth(0x0800) + ipv4(6, A, A, len(l4)) + l4
    rig = FlowRig(eng, capacity=16, pd={0: dict(drop_pack=1, land=1)}, syn_check=0)
    _, e = rig.step(*batch([land, rev]))
    assert statuses(e) == [LAND, FW] and (int(e["verdict"][1]) >> 16) & abi.F_NEWFLOW
    assert not (int(e["verdict"][1]) >> 16) & abi.F_TOCLIENT
    rig.close()
    # 8: across a tick syncount is the SYN-created flows; syn_count below it: every SYN is 27, live flows' included
    rig = FlowRig(eng, capacity=3, td={0: dict(drop_pack=1, syn_count=2)})
    fr = [frame("syn", A + i, B) for i in range(3)] + [syn, frame("syn", A + 1, B), frame("syn", A + 9, B)]
    _, e = rig.step(*batch(fr))
    assert statuses(e) == [FW] * 5 + [NOMEM] and accum(rig) == (0, 6, 3)
    rig.tick(NOW + 1)
    assert rig.m.atk.ai[0]["syncount"] == 3
    _, e = rig.step(*batch([syn, frame("syn", A + 20, B), frame("ack", A + 1, B)]), now=NOW + 1, outs=PART)
    assert statuses(e) == [SYNC, SYNC, FW]
    rig.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_batch_sizes(eng, n):
    """Tail lanes, a miss tile that is also the last tile, flows that recur across batches and seconds, every layout,
    ports 0-3 mixed in every tile, aging in between; then an arming packet in the last valid lane only."""
    rig = FlowRig(eng, pd=PD, td=TD, hold=2, capacity=max(4, n // 2))    # (the pool runs out: revokes as well)
    seen = set()
    for sec in range(5):
        for sub in range(2):
            hdr, lens, ports = mixed(n, 100 * n + 10 * (sec % 3) + sub)  # (seconds 3, 4 replay 0, 1: live flows)
            _, e = rig.step(hdr, lens, ports, now=NOW + sec, outs=LAYOUTS[(sec + sub) % 4], what=f"n {n} sec {sec}.{sub}")
            seen |= set(statuses(e))
        rig.tick(NOW + sec + 1)
        if sec == 2:
            rig.age(NOW + 30, 20)
    if n >= 63:
        assert {LAND, SYNF, SYNC, UDPF, NOMEM, NOSYN, FW} <= seen, seen
    rig.set(PD, TD, hold=7)
    for kind, field in (("udp", "udp_flood_hold"), ("syn", "syn_flood_hold")):
        rig.tick(NOW + 100)
        rig.tick(NOW + 100)                          # two quiet ticks: every pps 0, every hold released
        hdr, lens, _ = mixed(n, 7, only_last=kind)
        ports = np.zeros(n, np.uint8)
        rig.step(hdr, lens, ports, now=NOW + 100)    # pps was 0: counted, not dropped
        rig.tick(NOW + 101)
        rig.clock(NOW + 103)
        _, e = rig.step(hdr, lens, ports, now=NOW + 103)
        assert statuses(e)[-1] == (UDPF if kind == "udp" else SYNF)
        assert rig.m.atk.ai[0][field] == 1 and rig.m.atk.ai[0][field + "_time"] == NOW + 110
    rig.close()


def test_creator_and_dropped_syn_of_one_tuple(eng):
    """Port 0 drops every SYN (flood, armed by the first interval), port 1 drops none.  The same 5-tuple arrives on
    both: as creator and dropped SYN in one tile (both orders) and in different tiles (both orders).  A 5-tuple that
    appears only in dropped packets leaves no claim, no pending slot and no tombstone."""
    rig = FlowRig(eng, capacity=64, td={0: dict(FLOOD0, flood_udp=0)})
    rig.step(*batch([frame("syn", B, A)]), ports=np.zeros(1, np.uint8))
    rig.tick(NOW + 1)                                                  # port 0: synpps 1 > 0
    n = 130
    fr, ports = [frame("icmp", A + 50 + i, B) for i in range(n)], np.ones(n, np.uint8)
    place = {"W": (10, 11), "X": (13, 12), "Y": (5, 70), "Z": (71, 6)}   # tuple: (creator index, dropped index)
    for j, (cre, drp) in enumerate(place.values()):
        fr[cre] = fr[drp] = frame("syn", A + j, B)
        ports[drp] = 0
    for i in (20, 80, 129):                                              # only ever dropped
        fr[i], ports[i] = frame("syn", A + 9, B), 0
    _, e = rig.step(*batch(fr), ports=ports, now=NOW + 1)
    st = statuses(e)
    for cre, drp in place.values():
        assert st[cre] == FW and (int(e["verdict"][cre]) >> 16) & abi.F_NEWFLOW and st[drp] == SYNF
    assert [st[i] for i in (20, 80, 129)] == [SYNF] * 3
    fi = rig.check()
    assert fi["live"] == 5 and fi["tombstones"] == 0 and rig.m.atk.ai[1]["syncount_accum"] == 4
    assert not any(r[0] == A + 9 for r in table(eng.flow_dump()))
    rig.close()


@pytest.mark.parametrize("capacity,extra", [(8, 0), (48, 20), (64, 0)], ids=["revoke", "checked-fits", "unchecked"])
def test_revoke_counts_granted_creators(eng, capacity, extra):
    """40 new SYN flows in one batch (ports cycling 0-3, one port byte >= 4): capacity 8, the creators past the pool are
    revoked and only the eight granted ones (packet order) count, per port; capacity 48 with 20 repeats behind them,
    the host's bound forces finalize's overflow check and the exact count fits; capacity 64, no check."""
    rig = FlowRig(eng, capacity=capacity)
    fr = [frame("syn", A + i, B) for i in range(40)] + [frame("syn", A + i, B) for i in range(extra)]
    ports = (np.arange(40 + extra) % 4).astype(np.uint8)
    ports[5] = 4 + 1                                                   # (port & 3 = 1, as index 5 would have anyway)
    _, e = rig.step(*batch(fr), ports=ports, outs=SEP)
    granted = min(capacity, 40)
    assert statuses(e)[:40] == [FW] * granted + [NOMEM] * (40 - granted)
    want = [int(((np.arange(granted) % 4) == p).sum()) for p in range(4)]
    assert [rig.m.atk.ai[p]["syncount_accum"] for p in range(4)] == want
    assert [rig.atk.info()["ai"][p]["syncount_accum"] for p in range(4)] == want
    assert rig.check()["live"] == granted
    rig.step(*batch(fr), ports=ports, now=NOW + 1, outs=PART8)        # again: the granted flows are found
    rig.close()


def test_thresholds_holds_and_enable_words(eng):
    """Deterministic batches on both sides of udp_speed, syn_speed and syn_count (strict >), the hold released at
    now == hold_time, enable words 0 / 1 / 2.  The statuses are worked out by hand."""
    td = {1: dict(drop_pack=1, flood_udp=1, udp_speed=7), 2: dict(drop_pack=1, flood_syn=1, syn_speed=7, syn_count=1 << 30),
          3: dict(drop_pack=1, flood_syn=0, syn_count=5)}
    rig = FlowRig(eng, td=td, hold=50, capacity=256)
    fresh = iter(range(1, 1 << 20))

    def run(nu, ns, nc, now):
        """nu UDP on port 1, ns SYNs of one live flow on port 2 (synpps counts packets, not flows), nc SYNs of new
        flows on port 3 (syncount counts creations)."""
        fr = [frame("udp", A, B)] * nu + [frame("syn", A, B)] * ns + [frame("syn", A + next(fresh), B) for _ in range(nc)]
        _, e = rig.step(*batch(fr), ports=np.array([1] * nu + [2] * ns + [3] * nc, np.uint8), now=now)
        st = statuses(e)
        return set(st[:nu]), set(st[nu:nu + ns]), set(st[nu + ns:])
    fw = {FW}
    assert run(7, 7, 5, NOW) == (fw, fw, fw)
    rig.tick(NOW + 1)                                   # udppps 7, synpps 7, syncount 5: each equal to its threshold
    assert [rig.m.atk.ai[1]["udppps"], rig.m.atk.ai[2]["synpps"], rig.m.atk.ai[3]["syncount"]] == [7, 7, 5]
    assert rig.m.atk.ai[2]["syncount"] == 1             # port 2: seven SYNs, one flow
    assert run(8, 8, 6, NOW + 1) == (fw, fw, fw)        # equal passes
    rig.tick(NOW + 2)                                   # 8, 8, 6: each one above
    rig.clock(NOW + 2)
    assert run(3, 3, 3, NOW + 2) == ({UDPF}, {SYNF}, {SYNC})
    info = rig.atk.info()
    assert (info["udpflood_drop"], info["synflood_drop"], info["syncount_drop"], info["land_drop"]) == (3, 3, 3, 0)
    assert info["ai"][1]["udp_flood_hold_time"] == NOW + 52 and info["ai"][2]["syn_flood_hold_time"] == NOW + 52
    rig.tick(NOW + 3)                                   # pps 3, 3 but held; syncount 0: the count monitor lets go
    assert run(2, 2, 2, NOW + 3) == ({UDPF}, {SYNF}, fw)
    rig.tick(NOW + 51)                                  # still held (hold_time NOW + 52), pps 2
    assert run(1, 1, 0, NOW + 51)[:2] == ({UDPF}, {SYNF})
    rig.tick(NOW + 52)                                  # now == hold_time: released; pps 1 <= 7
    assert run(1, 1, 0, NOW + 52)[:2] == (fw, fw)
    # enable words: only 1 acts, on either half
    for v in (0, 1, 2):
        for dp in (0, 1, 2):
            on = v == 1 and dp == 1
            rig.set({0: dict(land=v, drop_pack=dp)}, {0: dict(flood_udp=v, udp_speed=0, flood_syn=v, syn_speed=0,
                                                               syn_count=1 << 30, drop_pack=dp)}, hold=0)
            rig.step(*batch([frame("udp", A, B), frame("syn", A, B)]), now=NOW + 60)
            rig.tick(NOW + 61)                          # udppps 1, synpps 1 on port 0; hold 0: nothing stays held
            _, e = rig.step(*batch([frame("udp", A, B), frame("syn", A, B), frame("syn", A + 1, A + 1)]), now=NOW + 61)
            assert statuses(e) == ([UDPF, SYNF, LAND] if on else [FW, FW, FW]), (v, dp)
            rig.tick(NOW + 62)
            rig.tick(NOW + 62)
    rig.close()


_world = {}


def kernel_world(nrules):
    """4,096 + 37 mixed packets over a recurring flow population, their ports, and the model's answers for three
    intervals (below threshold, arming, held), computed once per rule set and shared by the three workgroup sizes."""
    if nrules not in _world:
        rules = synth.make_rules(nrules, seed=nrules)
        pk = synth.make_flow_packets(4096 + 37, rules, n_flows=900, seed=41, kind="imix", stride=128, syn_frac=0.6,
                                     malformed_frac=0.05)
        hdr, lens = pk["hdr"].copy(), pk["len"].copy()
        for i in range(0, len(lens), 6):               # some land packets (untagged, ihl 5 rows only)
            if hdr[i, 12] == 0x08 and hdr[i, 14] == 0x45:
                hdr[i, 30:34] = hdr[i, 26:30]
        ports = np.random.default_rng(9).integers(0, 4, len(lens)).astype(np.uint8)
        o = pyoracle.Oracle(rules, default_action=abi.ACL_RULE_ACTION_FW)
        m = AttackFlowModel(o, 700, AttackModel(PD, TD, 1))
        exps, infos = [], []
        for sec in range(3):
            m.atk.clock(NOW + sec)
            exps.append(m.classify_batch(hdr, lens, ports, cfg=o.cfg(0, 1, NOW + sec)))
            m.atk.tick(NOW + sec + 1)
            infos.append((m.info(), table(m.ft.dump()), m.ft.stats()))
        assert all(m.atk.totals[k] > 0 for k in abi.ATTACK_TOTALS)
        st = np.concatenate([e["verdict"] & 0xFF for e in exps])
        assert (st == NOMEM).any() and (st == NOSYN).any()
        m.close()
        _world[nrules] = (rules, hdr, lens, ports, exps, infos)
    return _world[nrules]


@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("nrules,tune,image", [(128, dict(), "lds"), (128, dict(lds_image=0), "global"),
                                               (4096, dict(), "split")], ids=["lds", "global", "split"])
def test_all_nine_flow_kernels(eng, nrules, tune, image, block):
    """4,133 packets through each of the nine FLOW + ATK kernels (three image placements x three workgroup sizes,
    selected by tuning; ppe_launch_info reports the stateless plan, so the flow-table plan is read from the planner it
    is cached from): 128 rules fit a 256-thread workgroup's LDS share, 4,096 rules are split at every size.  Several
    workgroups' counts per port, several workgroups racing for each hold, a pool that runs out."""
    rules, hdr, lens, ports, exps, infos = kernel_world(nrules)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    old = eng.tuning()
    try:
        eng.tuning(block=block, **tune)
        img, t, p = eng.image(), abi.Tuning(**eng.tuning()), abi.Plan()
        assert eng.lib.ppe_plan_image(img.ctypes.data, len(img), C.byref(t), 1, C.byref(p)) == 0
        assert (("global", "lds", "split")[p.mode], p.block, p.pipe) == (image, block, 1), p.as_dict()
        rig = FlowRig(eng, rules, pd=PD, td=TD, hold=1, capacity=700, commit=False)
        rig.m.close()                                  # (the answers are kernel_world's; this rig's model is not run)
        th, tl, tp = to_dev(hdr, lens, ports)
        rig.atk.ports([tp])
        for sec, exp in enumerate(exps):
            rig.atk.clock(NOW + sec)
            eng.clear_counters()
            out = alloc(len(lens), LAYOUTS[sec])
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW + sec))
            torch.cuda.synchronize()
            compare(collect(out, len(lens)), exp, len(lens), f"{image} {block} sec {sec}")
            cnt = eng.counters()
            assert [cnt[c] for c in abi.COUNTERS] == exp["counters"].tolist()
            rig.atk.tick(NOW + sec + 1)
            want, tab, st = infos[sec]
            info = rig.atk.info()
            assert [{k: a[k] for k in abi.ATTACK_STATE_FIELDS} for a in info["ai"]] == want["ai"], sec
            assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}
            assert table(eng.flow_dump()) == tab
            fi = eng.flow_info()
            assert (fi["live"], fi["new_flow"], fi["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"])
        rig.atk.close()
        eng.flow_destroy()
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("stride", [64, 128, 144])
def test_decode_edge_corpus(eng, stride):
    """tests/decode_corpus.py through the FLOW + ATK kernels at three window widths: all-zero rules first (only the
    accumulators move), then land and both floods dropping on every port, then the reversed corpus on the live flows."""
    rules = synth.make_rules(256, seed=256)
    hdr256, lens, _ = dc.corpus(rules)
    hdr256 = hdr256.copy()
    for i in range(0, len(lens), 7):                   # some land frames (untagged, ihl 5 rows only)
        if hdr256[i, 12] == 0x08 and hdr256[i, 13] == 0x00 and hdr256[i, 14] == 0x45:
            hdr256[i, 30:34] = hdr256[i, 26:30]
    rev256 = dc.corpus(rules, reverse=True)[0]
    ports = (np.arange(len(lens)) % 4).astype(np.uint8)
    rig = FlowRig(eng, rules, default_action=1, capacity=1 << 14, max_batch=1 << 14)
    o = rig.o

    def run(h256, now, outs, what):
        e = dc.expected(o, h256, lens, stride, o.cfg(0, 1, now))
        return rig.step(np.ascontiguousarray(h256[:, :stride]), lens, ports, now=now, outs=outs, what=what, wide=h256,
                        punt=e["punt"], narrow_tuple=e["tuple"], tmask=e["tuple_mask"])[1]
    e0 = run(hdr256, NOW, SEP, "all-zero rules")
    assert len(e0["dropped"]) == 0 and sum(a["udp_accum"] + a["syn_accum"] for a in rig.m.atk.ai) > 100
    assert sum(a["syncount_accum"] for a in rig.m.atk.ai) > 0
    rig.set({p: dict(drop_pack=1, land=1) for p in range(4)}, {p: FLOOD0 for p in range(4)}, hold=5)
    rig.tick(NOW + 1)
    e1 = run(hdr256, NOW + 1, PART8, "everything dropping")
    st = e1["verdict"] & 0xFF
    assert (st == LAND).any() and (st == SYNF).any() and (st == UDPF).any()
    assert (st == ST["WINDOW_PUNT"]).any() == (stride == 64)   # (IPv4 options push the L4 header past a 64-B window)
    run(rev256, NOW + 2, SEP, "reversed, dropping")
    rig.tick(NOW + 10)
    rig.tick(NOW + 10)                                  # holds released (hold_time NOW + 6), every pps 0
    e3 = run(rev256, NOW + 10, PART, "reversed, quiet")
    assert ((e3["verdict"] >> 16) & abi.F_TOCLIENT).any()
    rig.close()


def test_set_and_tick_are_stream_ordered(eng):
    """ppe_attack_set and ppe_attack_tick enqueued between queued ppe_classify_flow calls, no synchronise in between:
    each takes effect exactly at its place in the stream."""
    rig = FlowRig(eng, hold=9, capacity=64)
    hdr, lens, ports = mixed(257, 3)
    th, tl, tp = to_dev(hdr, lens, ports)
    rig.atk.ports([tp])
    eng.clear_counters()
    outs, exps = [], []

    def enqueue():
        out = alloc(len(lens), PLAIN)
        eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
        outs.append(out)
        exps.append(rig.m.classify_batch(hdr, lens, ports, cfg=rig.o.cfg(0, 1, NOW)))
    enqueue()                                           # all-zero rules: only the accumulators move
    rig.set(PD, TD, hold=9)
    enqueue()                                           # rules on, pps still 0: land drops only
    rig.atk.tick(NOW + 1), rig.m.atk.tick(NOW + 1)
    enqueue()                                           # arming
    rig.set(PD, {p: dict(TD[p], drop_pack=0) for p in TD}, hold=9)
    enqueue()                                           # traffic half off: land only, the holds stay
    rig.atk.tick(NOW + 2), rig.m.atk.tick(NOW + 2)
    rig.set(PD, TD, hold=9)
    enqueue()                                           # held
    rig.atk.tick(NOW + 10), rig.m.atk.tick(NOW + 10)    # hold_time = NOW + 10: released
    enqueue()
    torch.cuda.synchronize()
    total = np.zeros(32, np.uint64)
    kinds = []
    for i, (out, e) in enumerate(zip(outs, exps)):
        compare(collect(out, len(lens)), e, len(lens), f"launch {i}")
        kinds.append(set(statuses(e)) & {LAND, SYNF, SYNC, UDPF})
        total += e["counters"]
    assert kinds[0] == set() and kinds[1] == {LAND} and {SYNF, UDPF} <= kinds[2] and kinds[3] == {LAND}
    assert {SYNF, UDPF} <= kinds[4]
    cnt = eng.counters()
    assert [cnt[c] for c in abi.COUNTERS] == total.tolist()
    rig.check()
    rig.close()


def test_aging_and_forced_rehash_between_monitored_batches(eng):
    """Flows aged out batch after batch until the tombstones force a rehash, the monitors dropping all the while: the
    table, the flow counters and the monitors' state stay the model's."""
    rules = synth.make_rules(32, seed=23)
    rig = FlowRig(eng, rules, pd=PD, td=TD, hold=2, capacity=2000, max_batch=4096)
    now = NOW
    for b in range(10):
        pk = synth.make_flow_packets(4096, rules, n_flows=1500, seed=300 + b, syn_frac=0.9)
        ports = np.random.default_rng(b).integers(0, 4, 4096).astype(np.uint8)
        rig.clock(now)
        rig.step(pk["hdr"], pk["len"], ports, now=now, outs=LAYOUTS[b % 4], what=f"batch {b}")
        now += 15
        rig.tick(now)
        rig.age(now, 20)
    fi = rig.check()
    assert fi["del_flow"] > 0 and fi["rehashes"] >= 1 and any(rig.m.atk.totals.values())
    rig.close()


def test_frozen_scenario(eng):
    """tests/golden/attack_flow_v1.npz (ticks and aging between the batches) on the GPU."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_attack_flow_golden as gen
    finally:
        sys.path.pop(0)
    g = np.load(GOLDEN / "attack_flow_v1.npz")
    rig = FlowRig(eng, pd=gen.PD, td=gen.TD, hold=gen.HOLD, capacity=gen.CAPACITY)
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
        hdr, lens = batch(gen.frames_of(kinds, land, host))
        got, _ = rig.step(hdr, lens, ports, now=now, outs=LAYOUTS[b % 4], what=f"batch {b}")
        for k in ("verdict", "flow_hash", "acl_hit"):
            assert np.array_equal(got[k], g[f"{k}{b}"]), (k, b)
        assert np.array_equal(gen.table(eng.flow_dump()), g[f"table{b}"]), b
        b += 1
    assert b == int(g["nbatch"][0])
    rig.close()


def flow_run(eng, th, tl, n, now=NOW, outs=SEP):
    eng.clear_counters()
    out = alloc(n, outs)
    eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, now))
    torch.cuda.synchronize()
    return collect(out, n), eng.counters(), table(eng.flow_dump())


def test_lifecycle_and_refusals(eng):
    """attach-flow then detach: byte-identical to a context that never had an object.  The exclusivity errors.  The
    stateless calls and ppe_classify_host do not see a flow-attached object.  PPE_ENOTSUP with a port-scan table,
    tracking on or an object attached with ppe_attack_attach, the table usable afterwards.  ppe_attack_destroy
    detaches; ppe_flow_destroy leaves the attachment; the steered path raises before any collective."""
    rules = synth.make_rules(256, seed=256)
    pk = synth.make_flow_packets(4096, rules, n_flows=600, seed=21, syn_frac=0.6)
    hdr, lens = pk["hdr"], pk["len"]
    ports = (np.arange(4096) % 4).astype(np.uint8)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    th, tl, tp = to_dev(hdr, lens, ports)
    lib, cfg = eng.lib, eng.cfg(0, 1, NOW)

    def stateless():
        eng.clear_counters()
        out = alloc(4096, SEP)
        eng.classify_torch(th, tl, out, cfg=cfg)
        torch.cuda.synchronize()
        return collect(out, 4096), eng.counters()
    # never had an object: two batches through a fresh table
    eng.flow_create(10_000, 4096)
    base = [flow_run(eng, th, tl, 4096, NOW + i) for i in range(2)]
    eng.flow_destroy()
    plain, plain_cnt = stateless()
    host_ref = eng.classify_host(hdr[:256], lens[:256], cfg=cfg)
    # flow-attached with dropping rules, one batch, detached: as if it had never been there
    eng.flow_create(10_000, 4096)
    atk = eng.attack(AttackModel(PD, TD, 5).cfg(), attach="flow")
    assert eng.attack_flow_attached is atk and getattr(eng, "attack_attached", None) is None
    atk.ports([tp])
    # stateless calls and the host path run the plain kernels while flow-attached
    got, cnt = stateless()
    for k in SEP:
        assert np.array_equal(got[k], plain[k]), k
    assert cnt == plain_cnt and not any(a["udp_accum"] + a["syn_accum"] for a in atk.info()["ai"])
    h = eng.classify_host(hdr[:256], lens[:256], cfg=cfg)
    assert all(np.array_equal(h[k], host_ref[k]) for k in host_ref)
    atk.detach_flow()
    assert eng.attack_flow_attached is None
    for i in range(2):
        g = flow_run(eng, th, tl, 4096, NOW + i)
        for k in SEP:
            assert np.array_equal(g[0][k], base[i][0][k]), (i, k)
        assert g[1] == base[i][1] and g[2] == base[i][2]
    assert not any(a["udp_accum"] + a["syn_accum"] + a["syncount_accum"] for a in atk.info()["ai"])
    # exclusivity: one object, one attachment point
    atk.attach_flow()
    assert lib.ppe_attack_attach(eng.ctx, atk.h) == abi.PPE_EINVAL
    assert b"detach first" in lib.ppe_last_error(eng.ctx)
    atk.detach_flow()
    atk.attach()
    assert lib.ppe_flow_attack_attach(eng.ctx, atk.h) == abi.PPE_EINVAL
    assert b"detach first" in lib.ppe_last_error(eng.ctx)
    # an object attached with ppe_attack_attach still refuses the flow path, before touching anything
    out = {k: torch.full((4096,), -7, dtype=torch.int32, device=DEV) for k in ("verdict", "flow_hash", "acl_hit")}
    b = abi.Batch(th.data_ptr(), tl.data_ptr(), None, 4096, 64)
    r = abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(), None, None, None,
                   None)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    live = eng.flow_info()["live"]

    def refused():
        assert lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), s) == abi.PPE_ENOTSUP
        torch.cuda.synchronize()
        assert (out["verdict"].cpu().numpy() == -7).all() and eng.flow_info()["live"] == live
    refused()
    atk.detach()
    other = Engine(0)
    try:                                                # an object of another context
        foreign = other.attack(attach=False)
        assert lib.ppe_flow_attack_attach(eng.ctx, foreign.h) == abi.PPE_EINVAL
        foreign.close()
    finally:
        other.close()
    atk.attach_flow()
    before = atk.info()
    ps = eng.portscan(capacity=64, max_batch=4096)
    refused()                                           # a port-scan table attached
    ps.close()
    eng.stream_tcp(1, 0, 0)
    refused()                                           # stream tracking on
    eng.stream_tcp(0, 0, 0)
    assert atk.info() == before
    from ppe.dist import DeviceSteerOps, steered_classify_flow
    with pytest.raises(PPEError, match="-95"):          # before any collective: no process group is needed to see it
        steered_classify_flow(DeviceSteerOps(eng), None, th, tl, cfg, 1, 0)
    assert atk.info() == before
    # ppe_flow_destroy leaves the attachment; without a table the call fails as it does today; a new table is monitored
    eng.flow_destroy()
    assert lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), s) != 0
    eng.flow_create(10_000, 4096)
    atk.tick(NOW + 1)
    g = flow_run(eng, th, tl, 4096, NOW + 1)
    assert sum(a["syn_accum"] + a["udp_accum"] for a in atk.info()["ai"]) > 0
    # ppe_attack_destroy detaches from the flow point: the next batches are the plain ones of a warm table
    atk.close()
    assert eng.attack_flow_attached is None
    eng.flow_destroy()
    eng.flow_create(10_000, 4096)
    g = flow_run(eng, th, tl, 4096, NOW)
    for k in SEP:
        assert np.array_equal(g[0][k], base[0][0][k]), k
    eng.flow_destroy()
