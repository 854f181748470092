"""The attack monitors with TCP sessions on the flow-table path (csrc/ppe_kernels_flow_stream_attack.hip;
ppe_flow_stream_monitors): after every batch, tick and aging step the per-packet outputs and lists (64 guard entries
behind each), the 32 counters, the 58 stream counters, ppe_flow_info, the flow dump, the session dump with the flow's
port byte and the whole ppe_attack_info equal tests/flow_stream_attack_model.py, whose syncount_accum takes the
reference's +1 and -1.  Integer work: no tolerance.  Shapes: 256 rules, a table of a few thousand slots, stride 144."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
import stream_session_corpus as sc  # noqa: E402
import stream_session_model as m  # noqa: E402
from attack_model import U64, AttackModel, frame  # noqa: E402
from attack_model import batch as frames_batch  # noqa: E402
from flow_stream_attack_model import FlowStreamAttackModel  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402
from stream_session_corpus import A, P, RS, S, c, s  # noqa: E402
from test_gpu_attack import PART, PART8, PLAIN, SEP, alloc, collect, compare, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

NOW = 1_700_000_000
FW = abi.ACL_RULE_ACTION_FW
STRIDE = 144
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
# port 0: nothing drops; port 1: the UDP flood at speed 0 (any traffic arms the next interval's first packet); port 2:
# the SYN flood past 3 a second; port 3: land
PD = {3: dict(drop_pack=1, land=1)}
TD = {1: dict(drop_pack=1, flood_udp=1, udp_speed=0, syn_count=1 << 30),
      2: dict(drop_pack=1, flood_syn=1, syn_speed=3, syn_count=1 << 30)}


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(scope="module")
def MAX(engines):
    return engines[0].flow_stream_max()


@pytest.fixture(scope="module")
def generated():
    """The generated conversations with UDP and land frames mixed in and a port byte per packet: computed once,
    shared, never changed (the tests slice and copy)."""
    seq = sc.generate()
    hdr, lens = sc.batch(seq, STRIDE, vlan_every=3)
    rng = np.random.default_rng(77)
    ports = rng.integers(0, 4, len(seq)).astype(np.uint8)
    extra = [frame("udp", 0x0A0A0000 + i, sc.SERVER_IP) for i in range(8)] + [frame("syn", 0x0B000000 + i, 0x0B000000 + i)
                                                                             for i in range(4)]
    eh, el = frames_batch(extra, STRIDE)
    for k, i in enumerate(range(5, len(seq), 17)):  # (a replaced TCP packet's flow simply misses it)
        hdr[i], lens[i] = eh[k % len(extra)], el[k % len(extra)]
    return hdr, lens, ports


def script(f, steps, cisn=1000, sisn=5000):
    return [(f, p) for p in sc.packets(steps, cisn, sisn)]


def frames(items, vlan_every=0):
    return sc.batch(items, STRIDE, vlan_every)


class Rig:
    """An engine with sessions attached, monitors flow-attached and the switch on; the model beside it."""

    def __init__(self, eng, rules=None, pd=None, td=None, hold=600, capacity=3000, max_batch=2048, switch=1,
                 sessions=True, monitors=True, tune=None):
        self.eng = eng
        self.rules = synth.make_rules(256, seed=21) if rules is None else rules
        if tune:
            eng.tuning(**tune)
        eng.commit(self.rules, default_action=FW)
        eng.flow_create(capacity, max_batch)
        eng.stream_tcp(track=1 if sessions else 0, reasm=0)
        if sessions:
            eng.flow_stream(1)
        eng.flow_stream_monitors(switch)
        eng.clear_counters()
        eng.clear_stream_track_counters()
        self.o = pyoracle.Oracle(self.rules, default_action=FW)
        self.m = FlowStreamAttackModel(self.o, capacity, AttackModel(pd, td, hold))
        self.atk = eng.attack(self.m.atk.cfg(), attach="flow" if monitors else False)
        self.sessions, self.monitors = sessions, monitors
        self.counters = np.zeros(32, np.int64)
        self.clock(NOW)

    def close(self):
        self.atk.close()
        self.eng.flow_stream_monitors(0)
        self.eng.flow_destroy()
        self.eng.stream_tcp(track=0)
        self.m.close()

    def clock(self, now):
        self.atk.clock(now)
        self.m.atk.clock(now)

    def tick(self, now, check=True):
        self.atk.tick(now)
        self.m.atk.tick(now)
        if check:
            self.same("after a tick")

    def set(self, pd=None, td=None, hold=600):
        self.m.atk.set(pd, td, hold)
        self.atk.set(self.m.atk.cfg())

    def age(self, now, timeout=20, what="after aging"):
        n = self.m.age(now, timeout)
        assert self.eng.flow_age(now, timeout) == n, what
        self.same(what)
        return n

    def expect(self, hdr, lens, ports, now, syn_check=1):
        exp, reasons = self.m.classify_batch(hdr, lens, ports, cfg=self.o.cfg(0, syn_check, now))
        self.counters += exp["counters"].astype(np.int64)
        return exp, reasons

    def enqueue(self, hdr, lens, ports, now, outs=SEP, syn_check=1):
        th, tl, tp = to_dev(hdr, lens, ports)
        self.atk.ports([tp] if tp is not None else None)
        out = alloc(len(lens), outs)
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, syn_check, now))
        return out, (th, tl, tp)

    def step(self, hdr, lens, ports=None, now=NOW, outs=SEP, syn_check=1, what="", kind=(6, 1)):
        n = len(lens)
        out, _ = self.enqueue(hdr, lens, ports, now, outs, syn_check)
        torch.cuda.synchronize()
        exp, reasons = self.expect(hdr, lens, ports, now, syn_check)
        compare(collect(out, n), exp, n, what)
        assert self.eng.flow_launch_info() == kind, what
        self.same(what)
        return exp, reasons

    def same(self, what=""):
        cnt = self.eng.counters()
        assert [cnt[k] for k in abi.COUNTERS] == self.counters[:len(abi.COUNTERS)].tolist(), what
        assert list(self.eng.stream_track_counters().values()) == self.m.cnt.c, what
        info, want = self.atk.info(), self.m.info()
        for p in range(4):
            g = {k: info["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
            if self.monitors:
                assert g == want["ai"][p], (what, "port", p, g, want["ai"][p])
            else:  # (an object that is not attached sees nothing)
                assert not any(g.values()), (what, "port", p, g)
        if self.monitors:
            assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}, what
        assert table(self.eng.flow_dump()) == table(self.m.ft.dump()), what
        fi, st = self.eng.flow_info(), self.m.ft.stats()
        assert (fi["live"], fi["new_flow"], fi["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        if not self.sessions:
            return
        got = {tuple(sorted(((e.sip, e.sport), (e.dip, e.dport)))):
               (e.state, e.flags) + e.client.astuple() + e.server.astuple() + (e.pad,) for e in self.eng.flow_stream_dump()}
        want = self.m.sessions()
        assert got == want, (what, [(k, got.get(k), want[k]) for k in want if got.get(k) != want[k]][:3])

    def accum(self):
        return [a["syncount_accum"] for a in self.m.atk.ai]


def key(f):
    cip, cport = sc.endpoints(f)
    return tuple(sorted(((cip, cport), (sc.SERVER_IP, sc.SERVER_PORT))))


def test_known_answers_one_packet_per_batch(engines):
    """tests/test_flow_stream_attack_model.py's cases (a), (b), (c), (e), (f), a batch of one packet each; the
    accumulators asserted here are the hand-derived ones, everything else is compared with the model by step()."""
    def one_by_one(rig, items, ports, now=NOW):
        sts = []
        for k, (it, pb) in enumerate(zip(items, ports)):
            exp, _ = rig.step(*frames([it]), np.array([pb], np.uint8), now=now, what=f"packet {k}")
            sts.append(int(exp["verdict"][0]) & 0xFF)
        return sts

    rig = Rig(engines[0])
    try:
        assert one_by_one(rig, script(1, sc.EST), [1, 2, 2]) == [0, 0, 0]                      # (a)
        assert rig.accum() == [0, 1, U64, 0]
        rig.tick(NOW + 1)
        assert [a["syncount"] for a in rig.m.atk.ai] == [0, 1, U64, 0]
        for k, syn_count in enumerate((0xFFFFFFFF, 0)):
            rig.set(td={2: dict(drop_pack=1, syn_count=syn_count)})
            assert one_by_one(rig, script(2 + k, sc.SYN_SENT), [2], NOW + 1) == [SYNC]
        rig.set()
        rig.tick(NOW + 2)
        rig.tick(NOW + 3)
        assert one_by_one(rig, script(10, sc.WHS4_RECV + [s(A, 1, 1, win=3000)]), [0, 1, 2, 3], NOW + 3) == [0] * 4  # (b)
        assert rig.accum() == [1, 0, 0, U64]
        rig.tick(NOW + 4)
        assert one_by_one(rig, script(11, sc.SYN_RECV + [c(A, 1, 2)]), [1, 1, 1], NOW + 4) == [0, 0, 29]  # (c)
        assert rig.accum() == [0, 1, 0, 0]
        rig.tick(NOW + 5)
        assert one_by_one(rig, script(12, sc.CONV_REUSE), [1] * 7 + [2], NOW + 5) == [0] * 8     # (e)
        assert rig.accum() == [0, 0, U64, 0]
        rig.tick(NOW + 6)
        rig.tick(NOW + 7)
        one_by_one(rig, script(13, sc.SYN_SENT), [2], NOW + 7)                                   # (f)
        rig.tick(NOW + 8)
        rig.set(td={2: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)})
        st = one_by_one(rig, script(14, sc.EST), [1, 2, 1], NOW + 8)
        assert st[:2] == [0, SYNF] and st[2] != 0 and rig.m.ssn[key(14)].state == m.TCP_SYN_SENT
        assert rig.accum() == [0, 1, 0, 0]
    finally:
        rig.close()


@pytest.mark.parametrize("ports", [[1, 1, 1], [1, 2, 3]], ids=["one port", "three ports"])
def test_a_whole_handshake_in_one_batch(engines, ports):
    """+1 and -1 in one launch."""
    rig = Rig(engines[0])
    try:
        rig.step(*frames(script(1, sc.EST)), np.array(ports, np.uint8), what="handshake")
        assert rig.accum() == ([0, 0, 0, 0] if ports[0] == ports[2] else [0, 1, 0, U64])
        assert rig.m.ssn[key(1)].state == m.TCP_ESTABLISHED
    finally:
        rig.close()


@pytest.mark.parametrize("outs", [SEP, PART, PART8, PLAIN], ids=["lists", "partition", "part8", "plain"])
def test_generated_conversations_every_size_and_layout(engines, generated, MAX, outs):
    """The generated sequence in batches of n in {1, 63, 64, 65, MAX} and the rest by MAX on one table, a tick between
    the batches: flows span batches and ports, the UDP hold is armed inside a batch, SYN|ACKs are dropped ahead of their
    sessions, the -1 lands on other ports than the +1."""
    hdr, lens, ports = generated
    rig = Rig(engines[0], pd=PD, td=TD, hold=2)
    seen = set()
    try:
        pos, sizes, k = 0, [1, 63, 64, 65, MAX], 0
        while pos < len(lens):
            n = min(sizes[k] if k < len(sizes) else MAX, len(lens) - pos)
            sl = slice(pos, pos + n)
            exp, _ = rig.step(hdr[sl], lens[sl], ports[sl], now=NOW + k, outs=outs, syn_check=0 if k % 3 == 2 else 1,
                              what=f"batch {k} n={n}")
            seen |= set((exp["verdict"] & 0xFF).tolist())
            pos, k = pos + n, k + 1
            rig.tick(NOW + k)
        assert {LAND, SYNF, UDPF, 0, 29} <= seen, seen
        assert any(a > (1 << 63) for a in rig.accum() + [x["syncount"] for x in rig.m.atk.ai])  # a gauge below zero
    finally:
        rig.close()


def test_max_completing_acks_on_one_port(engines, MAX):
    """MAX flows whose completing ACKs share one batch and one port: exactly -MAX, from MAX walkers' LDS adds."""
    rig = Rig(engines[0])
    try:
        ones = np.ones(MAX, np.uint8)
        rig.step(*frames([(i, m.Pkt(False, S, 1000 + i, 0, 1000)) for i in range(MAX)]), ones, what="SYNs")
        rig.step(*frames([(i, m.Pkt(True, S | A, 5000 + i, 1001 + i, 2000)) for i in range(MAX)]), ones, now=NOW + 1,
                 what="SYN|ACKs")
        assert rig.accum() == [0, MAX, 0, 0]
        rig.step(*frames([(i, m.Pkt(False, A, 1001 + i, 5001 + i, 1000)) for i in range(MAX)]), 2 * ones, now=NOW + 2,
                 what="ACKs")
        assert rig.accum() == [0, MAX, (0 - MAX) & U64, 0]
        assert all(x.state == m.TCP_ESTABLISHED for x in rig.m.ssn.values())
    finally:
        rig.close()


def test_one_flow_owning_the_batch(engines, MAX):
    """One flow's packets fill a whole batch (the longest walk), its handshake at the front."""
    rig = Rig(engines[0])
    try:
        steps, cs, ss = list(sc.EST), 1, 1
        while len(steps) < MAX:
            if len(steps) % 3:
                steps.append(c(A | P, cs, ss, plen=10))
                cs += 10
            else:
                steps.append(s(A | P, ss, cs, plen=20))
                ss += 20
        ports = (np.arange(MAX) % 4).astype(np.uint8)
        exp, r = rig.step(*frames(script(7, steps, 0xFFFFFF00, 0x7FFFFFF0)), ports, what="one flow x MAX")
        assert not r.any() and rig.m.ssn[key(7)].state == m.TCP_ESTABLISHED
        assert rig.accum() == [1, 0, U64, 0]  # the SYN on port 0, the completing ACK on port 2
    finally:
        rig.close()


def test_aging_every_state_then_again_then_created_again(engines):
    rig = Rig(engines[0])
    try:
        items, ports = [], []
        for f, (pre, state) in enumerate(sc.PREFIX_STATE + [(sc.SYN_SENT + [s(RS | A, 0, 1)], m.TCP_CLOSED)]):
            items += script(f, pre)
            ports += [f % 4] + [(f + 1) % 4] * (len(pre) - 1)
        h, ln = frames(items)
        uh, ul = frames_batch([frame("udp", 0x0A0A0001, sc.SERVER_IP), frame("ack", 0x0A0A0002, sc.SERVER_IP)], STRIDE)
        rig.step(np.vstack([h, uh]), np.concatenate([ln, ul]), np.array(ports + [1, 2], np.uint8), syn_check=0,
                 what="every state")
        states = {x.state for x in rig.m.ssn.values()}
        assert states >= {st for _, st in sc.PREFIX_STATE} | {m.TCP_NONE}
        before = rig.accum()
        n = rig.age(NOW + 100, 20, "aged")
        assert n >= len(sc.PREFIX_STATE) + 1 and rig.accum() != before
        assert rig.age(NOW + 200, 20, "aged again: tombstones") == 0
        rig.step(*frames(script(0, sc.SYN_RECV)), np.array([3, 3], np.uint8), now=NOW + 201, what="created again")
        assert rig.m.port[key(0)] == 3
        rig.age(NOW + 300, 20, "and aged in its handshake")
    finally:
        rig.close()


def test_rehash_between_a_syn_and_its_aging(engines):
    """Fillers in SYN_SENT age out 250 at a time (each a -1 on its own port) until the tombstones force a rehash; the
    kept flow's port byte moves with its record and takes its -1 when it ages at last."""
    rig = Rig(engines[0], capacity=300, max_batch=256)
    try:
        rig.step(*frames(script(5, sc.SYN_SENT, 0xFFFFFFF0, 9)), np.array([3], np.uint8), what="the SYN")
        before, k = rig.eng.flow_info()["rehashes"], 0
        rng = np.random.default_rng(3)
        while rig.eng.flow_info()["rehashes"] == before:
            k += 1
            assert k < 20
            filler = [(10_000 + 250 * k + i, m.Pkt(False, S, i, 0, 100)) for i in range(250)]
            rig.step(*frames(filler), rng.integers(0, 4, 250).astype(np.uint8), now=NOW + 40 * k, what=f"filler {k}")
            rig.step(*frames(script(5, [c(S, 0)], 0xFFFFFFF0, 9)), np.array([0], np.uint8), now=NOW + 40 * k + 25,
                     what="keep the flow alive")
            assert rig.age(NOW + 40 * k + 30, 20, f"aged {k}") == 250
            rig.tick(NOW + 40 * k + 31)
        assert rig.m.port[key(5)] == 3 and rig.accum() == [0, 0, 0, 0]
        assert rig.age(NOW + 40 * k + 100, 20, "the kept flow") == 1
        assert rig.accum() == [0, 0, 0, U64]
    finally:
        rig.close()


@pytest.mark.parametrize("nrules,tune,place", [(256, dict(), "lds"), (4096, dict(), "split"),
                                               (256, dict(lds_image=0), "global")])
def test_the_three_image_placements(engines, generated, MAX, nrules, tune, place):
    hdr, lens, ports = generated
    eng = engines[0]
    old = eng.tuning()
    try:
        rig = Rig(eng, rules=synth.make_rules(nrules, seed=nrules), pd=PD, td=TD, tune=tune)
        try:
            for k in range(2):
                sl = slice(k * MAX, (k + 1) * MAX)
                rig.step(hdr[sl], lens[sl], ports[sl], now=NOW + k, what=f"{place} {k}")
                rig.tick(NOW + k + 1)
        finally:
            rig.close()
    finally:
        eng.tuning(**old)


def test_300_batches_enqueued_without_a_synchronise(engines, generated):
    hdr, lens, ports = generated
    rig = Rig(engines[0], pd=PD, td=TD, hold=2)
    try:
        n, outs, keep, exps = 10, [], [], []
        for k in range(300):
            sl = slice(k * n, (k + 1) * n)
            if k % 25 == 24:
                rig.tick(NOW + k // 25 + 1, check=False)
            if k % 100 == 50:
                rig.set(PD, {**TD, 0: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)}, hold=3)
            out, dev = rig.enqueue(hdr[sl], lens[sl], ports[sl], NOW + k // 25)
            exps.append(rig.expect(hdr[sl], lens[sl], ports[sl], NOW + k // 25)[0])
            outs.append(out)
            keep.append(dev)
        torch.cuda.synchronize()
        for k, out in enumerate(outs):
            compare(collect(out, n), exps[k], n, f"batch {k}")
        rig.same("after 300 batches")
    finally:
        rig.close()


def test_every_refusal_leaves_everything(engines, generated, MAX):
    hdr, lens, ports = generated
    eng = engines[0]
    rig = Rig(eng, pd=PD, td=TD)
    ps = None
    try:
        rig.step(hdr[:300], lens[:300], ports[:300], what="before")

        def refused(code, h=hdr[300:400], ln=lens[300:400], pb=ports[300:400]):
            th, tl, tp = to_dev(h, ln, pb)
            rig.atk.ports([tp])
            out = alloc(len(ln), PLAIN)
            with pytest.raises(PPEError, match=str(code)):
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
            with pytest.raises(PPEError, match=str(code)):
                eng.classify_flow_host_ports(h, ln, pb, cfg=eng.cfg(0, 1, NOW), chunk=64)
            torch.cuda.synchronize()
            assert all((v.cpu().numpy() == -7).all() for v in out.values())
            rig.same(f"refused {code}")

        eng.flow_stream_monitors(0)
        refused(-95)  # the switch off: the refusal it always was
        with pytest.raises(PPEError, match="-22"):
            eng.flow_stream_monitors(2)
        eng.flow_stream_monitors(1)
        for able in (0, 1):
            ps = eng.portscan(attach="flow", able=able)
            refused(-95)
            ps.close()
            ps = None
        th, tl, tp = to_dev(hdr[:MAX + 1], lens[:MAX + 1], ports[:MAX + 1])
        rig.atk.ports([tp])
        out = alloc(MAX + 1, PLAIN)
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
        torch.cuda.synchronize()
        assert all((v.cpu().numpy() == -7).all() for v in out.values())
        rig.same("n = MAX + 1")
        refused(-22, np.ascontiguousarray(hdr[300:400, :128]))  # a header stride under 144 B
        eng.stream_tcp(track=1, reasm=1)
        refused(-95)
        eng.stream_tcp(track=1, reasm=0)
        with pytest.raises(PPEError, match="-95"):  # ppe_classify_flow_host keeps refusing monitors flow-attached
            eng.classify_flow_host(hdr[300:400], lens[300:400], cfg=eng.cfg(0, 1, NOW), chunk=64)
        rig.same("classify_flow_host")
        rig.step(hdr[300:400], lens[300:400], ports[300:400], now=NOW + 1, what="after the refusals")
    finally:
        if ps is not None:
            ps.close()
        rig.close()


def outputs_equal(x, y):
    return all(np.array_equal(x[q], y[q]) for q in ("verdict", "flow_hash", "acl_hit", "tuple"))


def test_switch_on_with_only_sessions_attached_is_kind_5(engines, generated):
    """The same kernel, kind and results as a twin context without the switch; the port byte stays 0."""
    hdr, lens, ports = generated
    a, b = Rig(engines[0], monitors=False, switch=1), Rig(engines[1], monitors=False, switch=0)
    try:
        for k in range(2):
            sl = slice(500 * k, 500 * (k + 1))
            x, y = (r.step(hdr[sl], lens[sl], None, now=NOW + k, what=f"sessions only {k}", kind=(5, 1))[0] for r in (a, b))
            assert outputs_equal(x, y)
        assert all(e.pad == 0 for e in a.eng.flow_stream_dump())
        for r in (a, b):
            r.age(NOW + 100, 20)  # (no object flow-attached: no decrement pass, nothing to count into)
    finally:
        a.close()
        b.close()


def test_switch_on_with_only_monitors_attached_is_kinds_0_and_4(engines, generated):
    hdr, lens, ports = generated
    a, b = (Rig(e, pd=PD, td=TD, sessions=False, switch=sw) for e, sw in zip(engines, (1, 0)))
    try:
        for r in (a, b):  # (no sessions: the model's table and monitors only)
            r.m.classify_batch = lambda h, ln, pb, cfg, r=r: (r.m.afm.classify_batch(h, ln, pb, cfg=cfg), None)
        sl = slice(0, 500)
        x, y = (r.step(hdr[sl], lens[sl], ports[sl], what="monitors only", kind=(0, 2))[0] for r in (a, b))
        assert outputs_equal(x, y)
        for r in (a, b):
            got = r.eng.classify_flow_host_ports(hdr[500:564], lens[500:564], ports[500:564], cfg=r.eng.cfg(0, 1, NOW),
                                                 chunk=64)
            exp, _ = r.expect(hdr[500:564], lens[500:564], ports[500:564], NOW)
            compare(got, exp, 64, "monitors only, host")
            assert r.eng.flow_launch_info() == (4, 1)
            r.same("monitors only, host")
            before = r.accum()
            assert r.eng.flow_age(NOW + 100, 20) == r.m.ft.age(NOW + 100, 20)  # (no sessions: nothing released)
            assert [x["syncount_accum"] for x in r.atk.info()["ai"]] == before
    finally:
        a.close()
        b.close()


def test_steered_path_refuses_before_its_first_collective(engines):
    from ppe import dist as pd

    class NoCollectives:
        def __getattr__(self, name):
            raise AssertionError(f"collective {name} reached")

    rig = Rig(engines[0])
    try:
        with pytest.raises(PPEError, match="-95"):
            pd.steered_classify_flow(pd.DeviceSteerOps(rig.eng), NoCollectives(), None, None, rig.eng.cfg(0, 1, NOW), 2, 0)
    finally:
        rig.close()
