"""The TCP session machine behind the flow table (csrc/ppe_kernels_flow_stream.hip; ppe_flow_stream_attach): after
every batch the per-packet outputs and lists (64 guard entries behind each), the 32 counters, the 58 stream counters,
ppe_flow_info, the flow dump and the session dump equal the oracle's sequential FlowHandlePacket with the serial model
of StreamTcpPacket (tests/stream_session_model.py) stepped behind it in packet order.  Integer work: no tolerance.
Shapes: 256 rules, a table of a few thousand slots, header stride 144."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
import stream_session_corpus as sc  # noqa: E402
import stream_session_model as m  # noqa: E402
from pktbuild import udp_packet  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from stream_session_corpus import A, P, S, c, s  # noqa: E402
from test_gpu_attack import PART, PART8, PLAIN, SEP, alloc, collect, compare, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

NOW = 1_000_000
FW = abi.ACL_RULE_ACTION_FW
STRIDE = 144
OUT_FW, OUT_DROP = abi.COUNTERS.index("out_fw"), abi.COUNTERS.index("out_drop")


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
    """The generated conversations, their frames and nothing else: computed once, shared, never changed."""
    seq = sc.generate()
    hdr, lens = sc.batch(seq, STRIDE, vlan_every=3)
    return seq, hdr, lens  # (the tests slice and copy; nobody writes into these)


def ends(t):
    """A flow's key whatever the direction: the two (address, port) ends, sorted."""
    return tuple(sorted(((int(t[0]), int(t[2]) & 0xFFFF), (int(t[1]), int(t[2]) >> 16))))


class Rig:
    """An engine with sessions attached, the oracle's flow table and the model's sessions beside it."""

    def __init__(self, eng, rules=None, default_action=FW, capacity=3000, max_batch=2048, commit=True, attach=True,
                 tune=None):
        self.eng = eng
        self.rules = synth.make_rules(256, seed=21) if rules is None else rules
        if tune:
            eng.tuning(**tune)
        if commit:
            eng.commit(self.rules, default_action=default_action)
        eng.flow_create(capacity, max_batch)
        eng.stream_tcp(track=1, reasm=0)
        self.attached = attach
        if attach:
            eng.flow_stream(1)
        eng.clear_counters()
        eng.clear_stream_track_counters()
        self.o = pyoracle.Oracle(self.rules, default_action=default_action)
        self.ft = pyoracle.OracleFlow(self.o, capacity=capacity)
        self.ssn, self.cnt = {}, m.Counters()
        self.counters = np.zeros(32, np.int64)

    def close(self):
        self.eng.flow_destroy()
        self.eng.stream_tcp(track=0)
        self.ft.close()

    def expect(self, hdr, lens, now, syn_check=1, track=True):
        """The oracle's flow path, then StreamTcpPacket for every TCP packet that has a flow, in index order."""
        ref = self.ft.classify_batch(hdr, lens, cfg=self.o.cfg(0, syn_check, now))
        v, cn = ref["verdict"].copy(), ref["counters"].astype(np.int64)
        reasons = np.zeros(len(lens), np.uint32)
        for i in np.flatnonzero(((v & 0xFF) == 0) & ((v >> 16) & (abi.F_FLOW | abi.F_TCP) == (abi.F_FLOW | abi.F_TCP))):
            fl, t = int(v[i]) >> 16, ref["tuple"][i]
            key = ends(t)
            if fl & abi.F_NEWFLOW or key not in self.ssn:
                self.ssn[key] = m.Session()
            if not track:
                continue
            row = hdr[i]
            th = 14 + (4 if (int(t[3]) >> 8) & 1 else 0)
            th += 4 * (int(row[th]) & 15)
            wso = (int(t[3]) >> 9) & 63
            p = m.Pkt(bool(fl & abi.F_TOCLIENT), int(row[th + 13]), int.from_bytes(row[th + 4:th + 8].tobytes(), "big"),
                      int.from_bytes(row[th + 8:th + 12].tobytes(), "big"),
                      int.from_bytes(row[th + 14:th + 16].tobytes(), "big"), int(t[3]) >> 16,
                      int(row[th + wso + 2]) if wso else None)
            r = m.step(self.ssn[key], p, self.cnt)
            if r:
                st = m.status_of(r)
                v[i] = st | (abi.ACT_DROP << 8) | ((fl | (r << abi.F_STREAM_REASON_SHIFT if st == 29 else 0)) << 16)
                cn[OUT_FW] -= 1
                cn[OUT_DROP] += 1
                reasons[i] = r
        self.counters += cn
        return dict(ref, verdict=v), reasons

    def enqueue(self, hdr, lens, now, outs=SEP, syn_check=1):
        th, tl, _ = to_dev(hdr, lens)
        out = alloc(len(lens), outs)
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, syn_check, now))
        return out, (th, tl)

    def step(self, hdr, lens, now=NOW, outs=SEP, syn_check=1, what="", kind=(5, 1)):
        n = len(lens)
        out, _ = self.enqueue(hdr, lens, now, outs, syn_check)
        torch.cuda.synchronize()
        exp, reasons = self.expect(hdr, lens, now, syn_check, track=kind == (5, 1))
        compare(collect(out, n), exp, n, what)
        assert self.eng.flow_launch_info() == kind, what
        self.same(what)
        return exp, reasons

    def same(self, what=""):
        cnt = self.eng.counters()
        assert [cnt[k] for k in abi.COUNTERS] == self.counters[:len(abi.COUNTERS)].tolist(), what
        assert list(self.eng.stream_track_counters().values()) == self.cnt.c, what
        dump = self.ft.dump()
        assert table(self.eng.flow_dump()) == table(dump), what
        info, st = self.eng.flow_info(), self.ft.stats()
        assert (info["live"], info["new_flow"], info["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        if not self.attached:  # (no session dump without sessions: PPE_EINVAL)
            with pytest.raises(PPEError, match="-22"):
                self.eng.flow_stream_dump()
            return
        want = {}
        for e in dump[dump["protocol"] == 6]:
            key = tuple(sorted(((int(e["sip"]), int(e["sport"])), (int(e["dip"]), int(e["dport"])))))
            want[key] = self.ssn.get(key, m.Session()).astuple()
        got = {tuple(sorted(((e.sip, e.sport), (e.dip, e.dport)))):
               (e.state, e.flags) + e.client.astuple() + e.server.astuple() for e in self.eng.flow_stream_dump()}
        assert got == want, (what, [k for k in want if got.get(k) != want[k]][:3])


def frames(items, vlan_every=0):
    return sc.batch(items, STRIDE, vlan_every)


def script(f, steps, cisn=1000, sisn=5000):
    return [(f, p) for p in sc.packets(steps, cisn, sisn)]


def test_known_answers_one_packet_per_batch(engines):
    """The complete conversation and the hand-derived rejections of tests/test_stream_session_model.py, a batch of one
    packet each, the statuses and reasons given here by hand."""
    rig = Rig(engines[0])
    try:
        for k, p in enumerate(script(1, sc.CONV_SERVER_CLOSES)):
            exp, r = rig.step(*frames([p]), what=f"conversation packet {k}")
            assert exp["verdict"][0] & 0xFFFF == 0 and r[0] == 0
        e = [x for x in rig.eng.flow_stream_dump()][0]
        assert (e.state, e.flags) == (m.TCP_CLOSED, m.F_3WHS_CONFIRMED)
        assert e.client.astuple() == (0x10, 0, 1000, 1102, 1102, 3101, 2000)
        assert e.server.astuple() == (0x10, 0, 5000, 5202, 5202, 6202, 1000)
        by_hand = [(sc.SYN_SENT + [s(S | A, 0, 2)], "WHS3_SYNACK_WITH_WRONG_ACK"),
                   (sc.SYN_RECV + [c(A, 1, 2)], "WHS3_RIGHT_SEQ_WRONG_ACK_EVASION"),
                   (sc.SYN_RECV + [c(A, 2, 2)], "WHS3_WRONG_SEQ_WRONG_ACK"),
                   (sc.EST + [c(A | P, 1, 1, plen=sc.SW + 1)], "EST_PACKET_OUT_OF_WINDOW"),
                   (sc.FIN_WAIT1 + [c(S, 0)], "SHUTDOWN_SYN_RESEND"),
                   ([c(S | A, 0, 1)], "MIDSTREAM_OR_ONESIDE_DISABLE")]
        for f, (steps, name) in enumerate(by_hand, start=10):
            for p in script(f, steps):
                exp, r = rig.step(*frames([p]), what=name)
            st = exp["verdict"][0] & 0xFF
            assert r[0] == m.R[name] and st == (22 if name.startswith("MIDSTREAM") else 29), name
            assert (int(exp["verdict"][0]) >> 26) == (0 if st == 22 else m.R[name])
    finally:
        rig.close()


def test_triggers_and_conversations_whole_in_one_batch(engines, MAX):
    """Every trigger and every conversation, each on its own flow and whole inside one batch: creators and their
    replies in the same batch, both directions interleaved within a wave."""
    rig = Rig(engines[0])
    try:
        items, f, seen = [], 100, set()
        for name, pre, steps in sc.TRIGGERS:
            items.append(script(f, pre + steps, *sc.ISNS[f % 4]))
            f += 1
        for conv in sc.CONVERSATIONS:
            items.append(script(f, conv, *sc.ISNS[f % 4]))
            f += 1
        batch, k = [], 0
        for it in items + [None]:
            if it is None or len(batch) + len(it) > MAX:
                exp, r = rig.step(*frames(batch, vlan_every=2), now=NOW + k, what=f"batch {k}")
                seen |= set(r.tolist())
                batch, k = [], k + 1
            if it:
                batch += it
        reach = {m.R[n] for n in m.FIELDS if n not in m.UNREACHABLE and n not in m.COUNT_ONLY}
        # (an ACK as a flow's first packet never has a flow under syn_check: MIDSTREAM_DISABLE is the next test's)
        assert seen - {0} == reach - {m.R["MIDSTREAM_DISABLE"]}
    finally:
        rig.close()


@pytest.mark.parametrize("outs", [SEP, PART, PART8, PLAIN], ids=["lists", "partition", "part8", "plain"])
def test_generated_conversations_every_size_and_layout(engines, generated, MAX, outs):
    """The generated sequence in batches of n in {1, 2, 63, 64, 65, MAX - 1, MAX} and the rest by MAX, on one table:
    flows span batches, walks of every length, every list layout; UDP and malformed packets between."""
    seq, hdr, lens = generated
    rig = Rig(engines[0])
    try:
        pos, sizes = 0, [1, 2, 63, 64, 65, MAX - 1, MAX]
        k = 0
        while pos < len(seq):
            n = min(sizes[k] if k < len(sizes) else MAX, len(seq) - pos)
            h, ln = hdr[pos:pos + n].copy(), lens[pos:pos + n].copy()
            if n >= 63:  # UDP and malformed packets between: they are untouched and do not reach a session
                u = np.frombuffer(udp_packet(0x0A0A0000 + k, sc.SERVER_IP, 999, 53), np.uint8)
                h[5], ln[5] = 0, len(u)
                h[5, :len(u)] = u
                h[9, 14] = 0x65  # IPv4 version 6: IPV4_VERSION_ERR
                h[11, 12:14] = (0x08, 0x06)  # ARP: L2_UNSUPPORT
            # (a replaced TCP packet's flow simply misses it: the model and the engine see the same sequence)
            rig.step(h, ln, now=NOW + k, outs=outs, syn_check=0 if k % 3 == 2 else 1, what=f"batch {k} n={n}")
            pos, k = pos + n, k + 1
        # (MIDSTREAM_DISABLE needs an ACK that creates its flow: the batches under syn_check 0)
        assert all(v >= (1 if m.FIELDS[i] == "MIDSTREAM_DISABLE" else 5) for i, v in enumerate(rig.cnt.c)
                   if m.FIELDS[i] not in m.UNREACHABLE)
    finally:
        rig.close()


def test_refusal_past_the_maximum_leaves_everything(engines, generated, MAX):
    seq, hdr, lens = generated
    rig = Rig(engines[0])
    try:
        rig.step(hdr[:200], lens[:200], what="first")
        th, tl, _ = to_dev(hdr[:MAX + 1], lens[:MAX + 1])
        out = alloc(MAX + 1, SEP)
        with pytest.raises(PPEError, match="-95"):
            rig.eng.classify_flow_torch(th, tl, out, cfg=rig.eng.cfg(0, 1, NOW))
        torch.cuda.synchronize()
        assert all((v.cpu().numpy() == -7).all() for v in out.values())
        rig.same("after the refusal")
        rig.step(hdr[200:200 + MAX], lens[200:200 + MAX], what="the table goes on")
    finally:
        rig.close()


@pytest.mark.parametrize("own", [1, 64, 65, "MAX"])
def test_one_flow_owning_the_batch(engines, MAX, own):
    """One flow's packets fill 1 / 64 / 65 / MAX places of a batch (the longest walk), data both ways across waves."""
    own = MAX if own == "MAX" else own
    rig = Rig(engines[0])
    try:
        steps = list(sc.EST)
        cs, ss = 1, 1
        while len(steps) < own + 3:
            if len(steps) % 3:
                steps.append(c(A | P, cs, ss, plen=10))
                cs += 10
            else:
                steps.append(s(A | P, ss, cs, plen=20))
                ss += 20
        pk = script(7, steps, 0xFFFFFF00, 0x7FFFFFF0)
        rig.step(*frames(pk[:3]), what="handshake")
        others = [(1000 + i, m.Pkt(False, S, 77 + i, 0, 512)) for i in range(MAX - own)]
        exp, r = rig.step(*frames(pk[3:3 + own] + others), now=NOW + 1, what=f"one flow x {own}")
        assert not r.any() and rig.ssn[ends((sc.endpoints(7)[0], sc.SERVER_IP, sc.endpoints(7)[1] | 80 << 16))].state == 4
    finally:
        rig.close()


def test_max_flows_of_one_packet_each_then_their_replies(engines, MAX):
    rig = Rig(engines[0])
    try:
        syn = [(i, m.Pkt(False, S, 1000 + i, 0, 1000, 0, 7 if i % 2 else None)) for i in range(MAX)]
        rig.step(*frames(syn), what="MAX creators")
        rep = [(i, m.Pkt(True, S | A, 5000 + i, 1001 + i + (i % 7 == 0), 2000)) for i in range(MAX)]
        exp, r = rig.step(*frames(rep), now=NOW + 1, what="MAX replies")
        assert (r != 0).sum() == len(range(0, MAX, 7)) and set(r.tolist()) == {0, m.R["WHS3_SYNACK_WITH_WRONG_ACK"]}
    finally:
        rig.close()


def test_aged_out_and_created_again(engines):
    """A flow in ESTABLISHED ages out; the same tuple's next SYN creates the flow again and its session starts at NONE
    (the PPE_F_NEWFLOW packet zeroes its slot's record; the table leaves the aged slot a tombstone until a rehash, so
    the new flow sits in the next slot of the probe sequence, and the slot arrays a rehash fills start zeroed);
    ppe_flow_age itself is as it was."""
    rig = Rig(engines[0])
    try:
        rig.step(*frames(script(3, sc.EST)), what="established")
        assert rig.eng.flow_stream_dump()[0].state == m.TCP_ESTABLISHED
        assert rig.eng.flow_age(NOW + 100, 20) == rig.ft.age(NOW + 100, 20) == 1
        assert rig.eng.flow_stream_dump() == []
        exp, r = rig.step(*frames(script(3, [c(S, 500)])), now=NOW + 101, what="again")
        e = rig.eng.flow_stream_dump()[0]
        assert (e.state, e.client.isn, e.client.last_ack, e.server.isn) == (m.TCP_SYN_SENT, 1500, 0, 0)
    finally:
        rig.close()


def test_rehash_between_the_packets_of_a_handshake(engines):
    """Flows are aged out until the tombstones force a rehash between a handshake's SYN|ACK and its ACK: the records
    move with their flows."""
    rig = Rig(engines[0], capacity=300, max_batch=256)
    try:
        rig.step(*frames(script(5, sc.SYN_RECV, 0xFFFFFFF0, 9)), what="SYN, SYN|ACK")
        before = rig.eng.flow_info()["rehashes"]
        k = 0
        while rig.eng.flow_info()["rehashes"] == before:
            k += 1
            assert k < 20
            filler = [(10_000 + 250 * k + i, m.Pkt(False, S, i, 0, 100)) for i in range(250)]
            rig.step(*frames(filler), now=NOW + 40 * k, what=f"filler {k}")
            rig.step(*frames(script(5, [c(S, 0)], 0xFFFFFFF0, 9)), now=NOW + 40 * k + 25, what="keep the flow alive")
            assert rig.eng.flow_age(NOW + 40 * k + 30, 20) == rig.ft.age(NOW + 40 * k + 30, 20) == 250
            rig.same(f"aged {k}")
        exp, r = rig.step(*frames(script(5, [c(A, 1, 1)], 0xFFFFFFF0, 9)), now=NOW + 40 * k + 31, what="the ACK")
        assert r[0] == 0 and rig.eng.flow_stream_dump()[0].state == m.TCP_ESTABLISHED
    finally:
        rig.close()


@pytest.mark.parametrize("nrules,tune,place", [(256, dict(), "lds"), (4096, dict(), "split"),
                                               (256, dict(lds_image=0), "global")])
def test_the_three_image_placements(engines, generated, MAX, nrules, tune, place):
    """256 rules fit a workgroup's LDS whole, 4,096 take the split placement (tests/test_gpu_flow.py), lds_image 0 reads
    the image from global memory."""
    seq, hdr, lens = generated
    eng = engines[0]
    old = eng.tuning()
    try:
        rig = Rig(eng, rules=synth.make_rules(nrules, seed=nrules), tune=tune)
        try:
            for k in range(2):
                rig.step(hdr[k * MAX:(k + 1) * MAX], lens[k * MAX:(k + 1) * MAX], now=NOW + k, what=f"{place} {k}")
        finally:
            rig.close()
    finally:
        eng.tuning(**old)


def test_300_batches_enqueued_without_a_synchronise(engines, generated):
    seq, hdr, lens = generated
    rig = Rig(engines[0])
    try:
        n, outs, keep = 10, [], []
        for k in range(300):
            out, dev = rig.enqueue(hdr[k * n:(k + 1) * n], lens[k * n:(k + 1) * n], NOW + k // 50)
            outs.append(out)
            keep.append(dev)
        torch.cuda.synchronize()
        for k, out in enumerate(outs):
            exp, _ = rig.expect(hdr[k * n:(k + 1) * n], lens[k * n:(k + 1) * n], NOW + k // 50)
            compare(collect(out, n), exp, n, f"batch {k}")
        rig.same("after 300 batches")
    finally:
        rig.close()


def test_track_toggled_with_flows_alive_and_attached_with_track_off(engines, generated):
    """Attached with track 0: byte-identical to a context that never attached (the plain kernels).  track 0 -> 1 with
    flows alive: every record zero, so the flows created meanwhile have no session."""
    seq, hdr, lens = generated
    a, b = Rig(engines[0]), Rig(engines[1], attach=False)
    try:
        for r in (a, b):
            r.eng.stream_tcp(track=0)
        for k in range(3):
            sl = slice(400 * k, 400 * (k + 1))
            x, y = (r.step(hdr[sl], lens[sl], now=NOW + k, what=f"track off {k}", kind=(1, 1))[0] for r in (a, b))
            assert all(np.array_equal(x[q], y[q]) for q in ("verdict", "flow_hash", "acl_hit", "tuple"))
        assert not any(a.eng.stream_track_counters().values())
        a.eng.stream_tcp(track=1, reasm=0)
        assert all(e.state == 0 and e.client.astuple() == (0,) * 7 for e in a.eng.flow_stream_dump())
        exp, r = a.step(hdr[1200:1700], lens[1200:1700], now=NOW + 3, what="track on again")
        assert r.any()  # packets of the flows alive meet a session at NONE: MIDSTREAM_DISABLE and its kin
    finally:
        a.close()
        b.close()


def test_every_refusal_leaves_the_table_and_the_counters(engines, generated):
    seq, hdr, lens = generated
    eng = engines[0]
    eng.flow_destroy()
    with pytest.raises(PPEError, match="-22"):
        eng.flow_stream(1)  # attach without a flow table
    rig = Rig(eng)
    ps = atk = None
    try:
        rig.step(hdr[:300], lens[:300], what="before")

        def refused(code, h=hdr[300:400], ln=lens[300:400], host=True):
            th, tl, _ = to_dev(h, ln)
            out = alloc(len(ln), PLAIN)
            with pytest.raises(PPEError, match=str(code)):
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
            if host:
                with pytest.raises(PPEError, match=str(code)):
                    eng.classify_flow_host(h, ln, cfg=eng.cfg(0, 1, NOW), chunk=64)
            torch.cuda.synchronize()
            assert all((v.cpu().numpy() == -7).all() for v in out.values())
            rig.same(f"refused {code}")

        for kw in (dict(reasm=1), dict(midstream=1), dict(async_oneside=1)):
            eng.stream_tcp(**dict(dict(track=1, reasm=0), **kw))
            refused(-95)
        eng.stream_tcp(track=1, reasm=0)
        ps = eng.portscan(attach="flow", able=0)
        refused(-95)
        ps.close()
        ps = None
        atk = eng.attack(attach="flow")
        refused(-95)
        atk.close()
        atk = None
        refused(-22, np.ascontiguousarray(hdr[300:400, :128]), lens[300:400])  # a header stride under 144 B
        eng.flow_stream(0)
        rig.attached = False
        refused(-95)  # tracking on without sessions: the refusal it always was
        eng.flow_stream(1)  # (zeroes the records: the model's sessions go with them)
        rig.attached, rig.ssn = True, {}
        rig.step(hdr[300:400], lens[300:400], now=NOW + 1, what="after the refusals")
    finally:
        for x in (ps, atk):
            if x is not None:
                x.close()
        rig.close()


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
