"""tests/flow_stream_portscan_model.py (the port-scan detector and the TCP sessions on one flow batch, without and with
the attack monitors: ppe_flow_stream_portscan, launch kinds 7 and 8) pinned on the CPU: against the kind-5 / kind-6 model
with the detector off, against the detector's models with tracking off, by hand-derived known answers (every accumulator
word and the final session records written out), by a generated sequence whose cases the test counts, and by one frozen
scenario.  The known answers and the generated sequence are also what the GPU tests run."""
import struct
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import flow_portscan_model as fpm
import portscan_model as psm
import pyoracle
import stream_session_corpus as sc
import stream_session_model as m
import test_flow_combined_model as tcm
import test_flow_portscan_model as tm
from attack_model import U64, AttackModel
from flow_combined_model import FlowCombinedModel
from flow_stream_attack_model import FlowStreamAttackModel, ends
from flow_stream_portscan_model import FlowStreamPortScanModel
from pktbuild import tcp_packet, udp_packet
from ppe import abi
from ppe.abi import ST
from stream_session_corpus import A, P, S, c, s

GOLDEN = Path(__file__).resolve().parent / "golden" / "flow_stream_portscan_v1.npz"
STRIDE = 144
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
OK, NOMEM, DETECTED, HOLD = psm.OK, psm.NOMEM, psm.DETECTED, psm.HOLD
P24, NOSYN, ADROP, AFW, FNOMEM = tm.P24, tm.NOSYN, tm.ADROP, tm.AFW, tm.FNOMEM
SYNF = ST["ATTACK_SYNFLOOD"]
SRV = sc.SERVER_IP
Z = (0, 0, 0, 0)
# the session records of the corpus' handshake with ISNs 1000 / 5000 and windows 1000 / 2000, by hand from stream-tcp.c:
#   SYN (StateNone :290-330)      state SYN_SENT; client.isn 1000, client.next_seq 1001; server.window = the SYN's 1000
#   SYN|ACK (3whs, :480-530)      state SYN_RECV; server.isn 5000, next_seq 5001, last_ack 5001; client.window 2000,
#                                 client.last_ack 1001, client.next_win 1001 + 2000; server.next_win 5001 + 1000
#   ACK (:640-662)                state ESTABLISHED; nothing else moves (seq 1001, ack 5001, the window unchanged)
#                (state, flags) + client (flags, wscale, isn, next_seq, last_ack, next_win, window) + server (the same)
R_SYN_SENT = (m.TCP_SYN_SENT, 0, 0, 0, 1000, 1001, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1000)
R_SYN_RECV = (m.TCP_SYN_RECV, 0, 0, 0, 1000, 1001, 1001, 3001, 2000, 0, 0, 5000, 5001, 5001, 6001, 1000)
R_EST = (m.TCP_ESTABLISHED,) + R_SYN_RECV[1:]
R_NONE = (0,) * 16


def script(f, steps, cisn=1000, sisn=5000):
    return [(f, p) for p in sc.packets(steps, cisn, sisn)]


def key(f):
    cip, cport = sc.endpoints(f)
    return ends(cip, SRV, cport, sc.SERVER_PORT)


def src(f):
    return sc.endpoints(f)[0]


def stack(items, stride=STRIDE):
    """A batch of corpus items (flow, Pkt) and raw frames, in order."""
    hdr = np.zeros((len(items), stride), np.uint8)
    lens = np.zeros(len(items), np.uint32)
    for i, it in enumerate(items):
        head, wire = (it, len(it)) if isinstance(it, bytes) else sc.frame(*it)
        hdr[i, :len(head)] = np.frombuffer(head, np.uint8)
        lens[i] = wire
    return hdr, lens


def kat_rules():
    """FW to ports 80-83 and 443 and from them (the replies); the default is DROP."""
    r = np.zeros(10, abi.RULE_DTYPE)
    for k, p in enumerate((80, 81, 82, 83, 443)):
        r[k]["sport_end"] = 65535
        r[k]["dport_start"] = r[k]["dport_end"] = p
        r[k + 5]["dport_end"] = 65535
        r[k + 5]["sport_start"] = r[k + 5]["sport_end"] = p
    r["protocol_end"] = 255
    r["action"] = FW
    return r


def make(kind, flow_capacity=100, ps_capacity=100, able=1, pd=None, td=None, track=1, rules=None, default=DROP,
         freq=3, hold=100, rate=1000, atk_hold=600):
    o = pyoracle.Oracle(kat_rules() if rules is None else rules, default_action=default)
    fp = fpm.FlowPortScanModel(o, flow_capacity, psm.PortScanModel(able, 0, freq, hold, ps_capacity, rate))
    return FlowStreamPortScanModel(o, fp, AttackModel(pd, td, atk_hold) if kind == 8 else None, track)


class Kat:
    """One model of kind 7 or 8 with the clocks and a step(): run a batch, return statuses, results and reasons."""

    def __init__(self, kind, **kw):
        self.kind, self.mod = kind, make(kind, **kw)
        self.now = 0

    def clock(self, cycles, seconds):
        self.mod.fp.ps.clock(cycles, seconds)
        if self.kind == 8:
            self.mod.atk.clock(seconds)
        self.now = seconds

    def step(self, items, ports=None, ts=None, syn_check=1):
        hdr, lens = stack(items)
        out, r = self.mod.classify_batch(hdr, lens, None if ports is None else np.array(ports, np.uint8),
                                         None if ts is None else np.array(ts, np.uint64),
                                         self.mod.o.cfg(0, syn_check, self.now))
        self.out = out
        return (out["verdict"] & 0xFF).tolist(), out["results"].tolist(), r.tolist()

    def age(self, now, timeout):
        return self.mod.age(now, timeout)

    def tick(self, now):
        self.mod.atk.tick(now)

    def set_rules(self, pd=None, td=None, hold=600):
        self.mod.atk.set(pd, td, hold)

    def words(self):
        return [(a["udp_accum"], a["syn_accum"], a["syncount"], a["syncount_accum"]) for a in self.mod.atk.ai]

    def stream(self):
        return {m.FIELDS[i]: v for i, v in enumerate(self.mod.cnt.c) if v}

    def hold(self, source):
        """tm.prime / tm.hot: four UDP packets to ports 9-12, then one to port 13 in the next window: DETECTED, the
        source held until ts 601 (tests/test_flow_portscan_model.py has the derivation).  Port 0, no flow, no session."""
        self.clock(10000, 500)
        assert self.step(tm.prime(source)["frames"])[0] == [ADROP] * 4
        self.clock(11500, 501)
        assert self.step(tm.hot(source)["frames"])[:2] == ([P24], [DETECTED])


@pytest.fixture(params=[7, 8], ids=["kind7", "kind8"])
def kind(request):
    return request.param


def kat_a_a_whole_handshake_in_one_batch(k):
    kind = k.kind
    k.clock(10000, 500)
    st, res, r = k.step(script(1, sc.EST), [1, 1, 2])
    # the SYN misses: PortScan_Detect once (first create, OK), FlowAdd; the SYN|ACK and the ACK find the flow
    # (flow.c:196-201) and are never at the detector
    assert st == [AFW] * 3 and res == [OK, -1, -1] and r == [0, 0, 0]
    assert k.mod.fp.ps.records() == {(src(1), 80, 0, 0, 10000, 10000, 0)}
    assert k.mod.sessions() == {key(1): R_EST + (1 if kind == 8 else 0,)}
    assert k.stream() == {"SYN_COUNT": 1, "SYN_ACK_COUNT": 1}
    if kind == 8:  # port 1: SYN and SYN|ACK (syn_accum), the creation's +1; port 2: the completing ACK's -1
        assert k.words() == [Z, (0, 2, 0, 1), (0, 0, 0, U64), Z]


def scan(k):
    """A scanner past the threshold: four SYNs to ports 80-83 in one window (first create, three port changes in the
    `< rate` branch: OK x 4, exception 3) create four flows; in the next window a SYN to port 443 rolls it
    (dp_portscan.c:177-194): last_exception 3 >= 3 and the port changed: DETECTED, hold 501 + 100; two more: HOLD."""
    x = 0x0A000055
    k.clock(10000, 500)
    st, res, r = k.step([tcp_packet(x, SRV, 40000, p) for p in (80, 81, 82, 83)], [3] * 4)
    assert st == [AFW] * 4 and res == [OK] * 4 and r == [0] * 4
    k.clock(11500, 501)
    st, res, r = k.step([tcp_packet(x, SRV, 40000, 443), tcp_packet(x, SRV, 40001, 80), tcp_packet(x, SRV, 40001, 80)],
                        [3] * 3)
    assert st == [P24] * 3 and res == [DETECTED, HOLD, HOLD] and r == [0] * 3
    return x


def kat_b_a_scanner_past_the_threshold_and_g_its_flows_aged_out(k):
    kind = k.kind
    x = scan(k)
    # pktbuild's SYN: seq 1, window 1024.  Four sessions in SYN_SENT; the status-24 SYNs have no flow, no session
    syn_sent = (m.TCP_SYN_SENT, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1024)
    port = 3 if kind == 8 else 0
    assert k.mod.sessions() == {ends(x, SRV, 40000, p): syn_sent + (port,) for p in (80, 81, 82, 83)}
    assert k.stream() == {"SYN_COUNT": 4}  # not 7
    assert len(k.mod.fp.flows) == 4 and k.mod.fp.ps.records() == {(x, 443, 1, 3, 11000, 11500, 601)}
    cn = dict(zip(abi.COUNTERS, k.out["counters"].tolist()))
    assert cn["out_drop"] == 3 and cn["out_fw"] == 0
    if kind == 8:  # seven SYNs at the monitor, four flows created by SYNs
        assert k.words() == [Z, Z, Z, (0, 7, 0, 4)]
    # (g) the half-open flows age out: StreamTcp_Flow_ResRelease, -1 each on the flow's port, once
    assert k.age(600, 20) == 4 and k.mod.sessions() == {}
    if kind == 8:
        assert k.words() == [Z, Z, Z, (0, 7, 0, 0)]
    assert k.age(700, 20) == 0
    if kind == 8:
        assert k.words() == [Z, Z, Z, (0, 7, 0, 0)]


def kat_c_a_syn_the_detector_drops_then_the_same_syn_creates(k):
    kind = k.kind
    k.hold(src(1))
    k.clock(14500, 502)
    # ts 600 < hold 601: HOLD, status 24; ts 601: the hold is over, the last branch (14500 - 11000 >= 2 rate), OK
    st, res, r = k.step(script(1, sc.SYN_SENT) * 2, [1, 2], ts=[600, 601])
    assert st == [P24, AFW] and res == [HOLD, OK] and r == [0, 0]
    assert (int(k.out["verdict"][1]) >> 16) & abi.F_NEWFLOW
    assert k.mod.sessions() == {key(1): R_SYN_SENT + (2 if kind == 8 else 0,)}  # word 13: the later packet's port
    assert k.stream() == {"SYN_COUNT": 1}
    if kind == 8:  # port 0: the five UDP packets of hold(); ports 1 and 2: a SYN each at the monitor; +1 on port 2 only
        assert k.words() == [(5, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1), Z]


def kat_d_a_creator_that_is_stream_dropped(k):
    kind = k.kind
    k.clock(10000, 500)
    st, res, r = k.step(script(1, [s(S | A, 0, 1), c(A, 1, 1)]), [2, 1])
    # the SYN|ACK has SYN: past syn_check, the detector under the server's record (OK), the ACL forwards source port 80,
    # FlowAdd; then StreamTcp with no session: MIDSTREAM_OR_ONESIDE_DISABLE (stream-tcp.c:275-283), status 22.  The flow
    # stays: the ACK finds it, and is dropped as well (no session, no SYN: MIDSTREAM_DISABLE, status 23)
    assert st == [22, 23] and res == [OK, -1]
    assert r == [m.R["MIDSTREAM_OR_ONESIDE_DISABLE"], m.R["MIDSTREAM_DISABLE"]]
    fl = [int(v) >> 16 for v in k.out["verdict"]]
    assert fl[0] & abi.F_NEWFLOW and fl[0] & abi.F_FLOW and fl[1] & abi.F_FLOW and not fl[1] & abi.F_NEWFLOW
    assert fl[1] & abi.F_TOCLIENT  # the flow is oriented as its creator, the server's packet
    assert [(int(v) >> 8) & 0xFF for v in k.out["verdict"]] == [abi.ACT_DROP] * 2
    assert len(k.mod.fp.flows) == 1 and k.mod.fp.ps.records() == {(SRV, sc.endpoints(1)[1], 0, 0, 10000, 10000, 0)}
    assert k.mod.sessions() == {key(1): R_NONE + (2 if kind == 8 else 0,)}
    assert k.stream() == {"SYN_ACK_COUNT": 1, "MIDSTREAM_OR_ONESIDE_DISABLE": 1, "MIDSTREAM_DISABLE": 1}
    cn = dict(zip(abi.COUNTERS, k.out["counters"].tolist()))
    assert cn["out_drop"] == 2 and cn["out_fw"] == 0 and cn["flow_proc_ok"] == 2
    if kind == 8:  # FlowAdd runs before StreamTcp: the SYN|ACK's +1 stays
        assert k.words() == [Z, Z, (0, 1, 0, 1), Z]


def kat_e_flow_nomem_after_the_detector_said_ok(k):  # (flow_capacity 1)
    kind = k.kind
    k.clock(10000, 500)
    st, res, r = k.step(script(1, sc.SYN_SENT) + script(2, sc.SYN_SENT), [1, 2])
    assert st == [AFW, FNOMEM] and res == [OK, OK] and r == [0, 0]
    assert k.mod.sessions() == {key(1): R_SYN_SENT + (1 if kind == 8 else 0,)} and key(2) not in k.mod.ssn
    assert k.stream() == {"SYN_COUNT": 1}
    assert k.mod.fp.ps.records() == {(src(1), 80, 0, 0, 10000, 10000, 0), (src(2), 80, 0, 0, 10000, 10000, 0)}
    if kind == 8:
        assert k.words() == [Z, (0, 1, 0, 1), (0, 1, 0, 0), Z]


def kat_f_a_data_packet_of_an_established_flow_whose_source_is_held(k):
    kind = k.kind
    x = src(1)
    k.clock(10000, 500)
    st, res, r = k.step(script(1, sc.EST) + [udp_packet(x, SRV, 5000, p) for p in (9, 10, 11)])
    assert st == [AFW] * 3 + [ADROP] * 3 and res == [OK, -1, -1, OK, OK, OK]
    k.clock(11500, 501)
    st, res, r = k.step([tcp_packet(x, SRV, 40001, 80)] + script(1, sc.EST + [c(A | P, 1, 1, plen=10)])[3:])
    # the new tuple's SYN rolls the window: DETECTED, the source is held; the data packet finds its flow: the session
    # steps (client.next_seq 1001 + 10), the detector does not
    assert st == [P24, AFW] and res == [DETECTED, -1] and r == [0, 0]
    assert k.mod.fp.ps.records() == {(x, 80, 1, 3, 11000, 11500, 601)}
    assert k.mod.sessions() == {key(1): R_EST[:5] + (1011,) + R_EST[6:] + (0,)}
    if kind == 8:  # all on port 0: three UDP packets; SYN, SYN|ACK and the dropped SYN; +1 at the creation, -1 at the ACK
        assert k.words() == [(3, 3, 0, 0), Z, Z, Z]


def kat_h_a_monitor_dropped_synack_leaves_syn_sent(k):  # (kind 8 only)
    k.clock(10000, 500)
    k.step(script(9, sc.SYN_SENT), [2])
    k.tick(501)
    assert k.words() == [Z, Z, (0, 0, 1, 0), Z] and k.mod.atk.ai[2]["synpps"] == 1
    k.set_rules(td={2: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)})
    k.clock(10000, 501)
    st, res, r = k.step(script(1, sc.EST), [1, 2, 1])
    # the SYN|ACK dies at the SYN-flood monitor: neither table, nor the detector, nor its session sees it; the ACK finds
    # the flow and meets SYN_SENT
    assert st[:2] == [AFW, SYNF] and res == [OK, -1, -1] and st[2] == 29 and r[2] != 0
    assert k.mod.sessions()[key(1)] == R_SYN_SENT + (1,)
    assert k.words() == [Z, (0, 1, 0, 1), (0, 1, 1, 0), Z]


# name -> (the case, the kinds it runs under, the model's arguments)
KATS = {"a": (kat_a_a_whole_handshake_in_one_batch, (7, 8), {}),
        "b_g": (kat_b_a_scanner_past_the_threshold_and_g_its_flows_aged_out, (7, 8), {}),
        "c": (kat_c_a_syn_the_detector_drops_then_the_same_syn_creates, (7, 8), {}),
        "d": (kat_d_a_creator_that_is_stream_dropped, (7, 8), {}),
        "e": (kat_e_flow_nomem_after_the_detector_said_ok, (7, 8), dict(flow_capacity=1)),
        "f": (kat_f_a_data_packet_of_an_established_flow_whose_source_is_held, (7, 8), {}),
        "h": (kat_h_a_monitor_dropped_synack_leaves_syn_sent, (8,), {})}
KAT_CASES = [(name, kd) for name in sorted(KATS) for kd in KATS[name][1]]


@pytest.mark.parametrize("name,kd", KAT_CASES, ids=[f"{n}-kind{k}" for n, k in KAT_CASES])
def test_known_answers(name, kd):
    case, _, kw = KATS[name]
    case(Kat(kd, **kw))


# ---- equivalences ----
def conv_batches():
    """The session corpus' generated conversations in batches of 300 with a port byte per packet."""
    seq = sc.generate()
    hdr, lens = sc.batch(seq, STRIDE, vlan_every=3)
    ports = np.random.default_rng(5).integers(0, 4, len(seq)).astype(np.uint8)
    return [(hdr[i:i + 300], lens[i:i + 300], ports[i:i + 300]) for i in range(0, 3000, 300)]


def test_detector_off_and_zero_rules_equal_the_kind_5_and_6_model(kind):
    """able = 0 and all-zero monitor rules: tests/flow_stream_attack_model.py's model (with all-zero rules its rows are
    the plain flow path's: kind 5's), rows, counters, sessions, stream counters and accumulators."""
    o = pyoracle.Oracle(np.zeros(0, abi.RULE_DTYPE), default_action=FW)
    ref = FlowStreamAttackModel(o, 200, AttackModel())
    mod = make(kind, flow_capacity=200, able=0, rules=np.zeros(0, abi.RULE_DTYPE), default=FW)
    for b, (hdr, lens, ports) in enumerate(conv_batches()):
        for x in (ref.atk, mod.atk if kind == 8 else None):
            if x is not None:
                x.clock(1000 + b)
        cfg = o.cfg(0, 1, 1000 + b)
        want, wr = ref.classify_batch(hdr, lens, ports if kind == 8 else None, cfg=cfg)
        got, gr = mod.classify_batch(hdr, lens, ports, None, cfg)
        for f in ("verdict", "flow_hash", "acl_hit", "tuple", "counters"):
            assert np.array_equal(got[f], want[f]), (b, f)
        assert np.array_equal(gr, wr) and mod.cnt.c == ref.cnt.c and (got["results"] == -1).all()
        assert mod.sessions() == ref.sessions()
        if kind == 8:
            assert mod.atk.info() == ref.atk.info()
        if b % 3 == 2:
            assert mod.age(1000 + b + 30, 20) == ref.age(1000 + b + 30, 20, release=kind == 8)
    assert sum(ref.cnt.c) > 100 and not mod.fp.ps.table
    ref.close()


def test_tracking_off_equals_the_detector_models(kind):
    seq, par = generated()
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)

    def fp():
        return fpm.FlowPortScanModel(o, par["flow_capacity"], psm.PortScanModel(1, 0, par["freq"], par["hold"],
                                                                               par["ps_capacity"], par["rate"]))
    ref = FlowCombinedModel(o, AttackModel(tcm.GEN_PD, tcm.GEN_TD, tcm.GEN_HOLD), fp()) if kind == 8 else fp()
    mod = FlowStreamPortScanModel(o, fp(), AttackModel(tcm.GEN_PD, tcm.GEN_TD, tcm.GEN_HOLD) if kind == 8 else None, track=0)
    for b, q in enumerate(seq[:25]):
        for ps in ((ref.fp.ps if kind == 8 else ref.ps), mod.fp.ps):
            ps.clock(q["now_c"], q["now_s"])
        if kind == 8:
            ref.atk.clock(q["now_s"])
            mod.atk.clock(q["now_s"])
        cfg = o.cfg(0, 1, q["now_s"])
        want = (ref.classify_batch(q["hdr"], q["lens"], q["ports"], q["ts"], cfg) if kind == 8 else
                ref.classify_batch(q["hdr"], q["lens"], q["ts"], cfg))
        got, r = mod.classify_batch(q["hdr"], q["lens"], q["ports"], q["ts"], cfg)
        for f in ("verdict", "flow_hash", "acl_hit", "tuple", "counters", "results"):
            assert np.array_equal(got[f], want[f]), (b, f)
        assert not r.any() and not sum(mod.cnt.c)
        assert mod.table() == ref.table()


# ---- the generated sequence of the GPU tests ----
SRC8 = [0x0A000000 + 16 * k + 1 for k in range(8)]
SRV2 = [0x0B000001, 0x0B000002]
FWPORTS = fpm.PORTS[:5]
L2 = bytes([2, 0x11, 0x22, 0x33, 0x44, 0x55, 2, 0x66, 0x77, 0x88, 0x99, 0xAA]) + struct.pack(">H", 0x0800)


def tcp_frame(sip, dip, sport, dport, flags, seq, ack, win=1000, plen=0):
    """sc.frame's TCP frame between any two ends: (the header bytes, the wire length)."""
    tcp = struct.pack(">HHIIBBHHH", sport, dport, seq & m.M32, ack & m.M32, 5 << 4, flags, win, 0, 0)
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 40 + plen, 0x1234, 0, 64, 6, 0, sip, dip)
    head = L2 + ip + tcp
    return head, len(head) + plen


def gen_sequence(seed, batches, max_n, flow_capacity=96):
    """The combined model's population (8 sources, two servers, five forwarded ports and one without a rule, four client
    ports) carrying conversations: per batch strands interleaved at random with each strand's order kept: whole handshakes
    with data, lone SYNs, a SYN|ACK first and its ACK, a source's SYNs across every port with a repeat later in the batch,
    UDP packets, and later packets of the connections earlier batches opened.  ts ascends inside a batch over three
    seconds (the detector's hold is two: a hold set early in a batch ends inside it).  Per batch (hdr, lens, ts, ports,
    now_s, now_c, age, tick)."""
    rng = np.random.default_rng(seed)
    now_s, now_c, last = 1000, 10 * fpm.RATE, None
    open_conns, out = [], []
    for b in range(batches):
        n = int(rng.integers(1, max_n + 1)) if b % 5 else int(rng.choice([1, 63, 64, 65, max_n - 1, max_n]))
        strands = []
        for q in open_conns:  # the connections of the batch before: data from both ends, now and then a FIN
            cip, sip, cp, sp, ci, si = q
            strands.append([tcp_frame(cip, sip, cp, sp, A | P, ci + 1, si + 1, plen=20),
                            tcp_frame(sip, cip, sp, cp, A, si + 1, ci + 21, win=2000)])
        open_conns = []
        total = sum(len(x) for x in strands)
        while total < n:
            cip, sip = SRC8[int(rng.integers(8))], SRV2[int(rng.integers(2))]
            cp, sp = 40000 + int(rng.integers(4)), FWPORTS[int(rng.integers(5))]
            ci, si = int(rng.integers(1 << 32)), int(rng.integers(1 << 32))
            syn = tcp_frame(cip, sip, cp, sp, S, ci, 0)
            synack = tcp_frame(sip, cip, sp, cp, S | A, si, ci + 1, win=2000)
            ack = tcp_frame(cip, sip, cp, sp, A, ci + 1, si + 1)
            u = rng.random()
            if u < 0.22:
                st = [syn, synack, ack, tcp_frame(cip, sip, cp, sp, A | P, ci + 1, si + 1, plen=20)]
            elif u < 0.32:
                st = [syn, synack, ack]
                open_conns.append((cip, sip, cp, sp, ci, si))
            elif u < 0.45:
                st = [syn]
            elif u < 0.55:
                st = [synack, ack]
            elif u < 0.75:  # a scan, and the first SYN again at its end
                ports = [fpm.PORTS[j] for j in rng.permutation(6)]
                st = [tcp_frame(cip, sip, cp, p, S, ci, 0) for p in ports]
                st.append(st[0])
            else:
                f = udp_packet(cip, sip, cp, fpm.PORTS[int(rng.integers(6))])
                st = [(f, len(f))]
            strands.append(st)
            total += len(st)
        order = np.repeat(np.arange(len(strands)), [len(x) for x in strands])
        rng.shuffle(order)
        pos, frames = [0] * len(strands), []
        for k in order.tolist()[:n]:
            frames.append(strands[k][pos[k]])
            pos[k] += 1
        hdr = np.zeros((n, STRIDE), np.uint8)
        lens = np.zeros(n, np.uint32)
        for i, (head, wire) in enumerate(frames):
            hdr[i, :len(head)] = np.frombuffer(head, np.uint8)
            lens[i] = wire
        now_c += int(rng.choice([0, fpm.RATE // 3, fpm.RATE + fpm.RATE // 2, 3 * fpm.RATE, 25 * fpm.RATE],
                                p=[0.3, 0.3, 0.3, 0.06, 0.04]))
        now_s += int(rng.integers(0, 3))
        ts = np.sort(now_s + rng.integers(0, 3, n)).astype(np.uint64)
        out.append(dict(hdr=hdr, lens=lens, ts=ts, ports=rng.integers(0, 4, n).astype(np.uint8), now_s=now_s, now_c=now_c,
                        age=(b % 4 == 3), tick=last is not None and now_s != last))
        last = now_s
    return out, dict(freq=2, flow_capacity=flow_capacity, ps_capacity=8, hold=2, rate=fpm.RATE)


SEED, BATCHES, MAX_N = 4711, 60, 130
NEEDED = ("a", "b", "c", "d", "e", "f")
_cache = {}


def generated():
    if "seq" not in _cache:
        _cache["seq"] = gen_sequence(SEED, BATCHES, MAX_N)
    return _cache["seq"]


def gen_model(par, kind, pd=tcm.GEN_PD, td=tcm.GEN_TD):
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    fp = fpm.FlowPortScanModel(o, par["flow_capacity"], psm.PortScanModel(1, 0, par["freq"], par["hold"],
                                                                         par["ps_capacity"], par["rate"]))
    return o, FlowStreamPortScanModel(o, fp, AttackModel(pd, td, tcm.GEN_HOLD) if kind == 8 else None)


def tally(ev, mod, held_before, q, out, reasons):
    """Counts the cases (a)-(f) of the known answers in one batch's result."""
    st, fl = out["verdict"] & 0xFF, out["verdict"] >> 16
    n = len(st)
    tup = [tuple(int(x) for x in out["tuple"][i]) for i in range(n)]
    fkey = [fpm.flow_key(t[0], t[1], t[2] & 0xFFFF, t[2] >> 16, t[3] & 0xFF) for t in tup]
    tcp = [(t[3] & 0xFF) == 6 for t in tup]
    sess = mod.sessions()
    half_open = Counter()
    for f in mod.fp.flows.values():
        e = ends(f["sip"], f["dip"], f["sport"], f["dport"])
        if f["protocol"] == 6 and sess[e][0] == m.TCP_SYN_SENT:
            half_open[f["sip"]] += 1
    dropped24 = {}
    for i in range(n):
        new = bool(fl[i] & abi.F_NEWFLOW)
        if st[i] == P24 and tcp[i]:
            dropped24.setdefault(fkey[i], i)
            if half_open[tup[i][0]]:
                ev["b"] += 1
        if new and tcp[i]:
            e = ends(tup[i][0], tup[i][1], tup[i][2] & 0xFFFF, tup[i][2] >> 16)
            if st[i] == AFW and out["results"][i] == OK and e in sess and sess[e][0] == m.TCP_ESTABLISHED:
                ev["a"] += 1
            if fkey[i] in dropped24 and dropped24[fkey[i]] < i:
                ev["c"] += 1
            if reasons[i]:
                ev["d"] += 1
        if st[i] == FNOMEM and tcp[i] and out["results"][i] == OK:
            ev["e"] += 1
        if (tcp[i] and (fl[i] & abi.F_FLOW) and not new and out["results"][i] == -1 and
                held_before.get(tup[i][0], 0) > int(q["ts"][i])):
            ev["f"] += 1  # (ts ascends: a hold that covers ts[i] as the batch starts was not released before packet i)


def run_generated(seq, par, kind, ev=None):
    """The model over the sequence: per batch (result, reasons); the model itself."""
    o, mod = gen_model(par, kind)
    outs = []
    for q in seq:
        if kind == 8:
            if q["tick"]:
                mod.atk.tick(q["now_s"])
            mod.atk.clock(q["now_s"])
        mod.fp.ps.clock(q["now_c"], q["now_s"])
        held = {sip: pcb["hold"] for sip, pcb in mod.fp.ps.table.items() if pcb["hold"]}
        out, r = mod.classify_batch(q["hdr"], q["lens"], q["ports"], q["ts"], o.cfg(0, 1, q["now_s"]))
        outs.append((out, r))
        if ev is not None:
            tally(ev, mod, held, q, out, r)
        if q["age"]:
            mod.age(q["now_s"], 2)
            mod.fp.ps.timeout(q["now_c"])
    return outs, mod


def test_generated_sequence_holds_every_case(kind):
    """A condition on the inputs, from the model alone: each of the cases (a)-(f) occurs at least 10 times, with the
    monitors and without; flows age out, stream drops occur, and with the monitors the gauge moves both ways."""
    seq, par = generated()
    ev = Counter()
    outs, mod = run_generated(seq, par, kind, ev)
    assert all(ev[k] >= 10 for k in NEEDED), dict(ev)
    st = np.concatenate([o["verdict"] & 0xFF for o, _ in outs])
    assert {P24, FNOMEM, NOSYN, ADROP, AFW, 29} <= set(st.tolist())
    assert mod.fp.del_flow >= 10 and sum(int(r.astype(bool).sum()) for _, r in outs) >= 10
    assert mod.cnt.c[m.R["SYN_COUNT"]] >= 10 and mod.cnt.c[m.R["SYN_ACK_COUNT"]] >= 10
    if kind == 8:
        assert {ST["ATTACK_LAND"], ST["ATTACK_UDPFLOOD"], ST["ATTACK_SYNCOUNT"]} & set(st.tolist())


def test_frozen_scenario():
    """One generated scenario frozen as model output (tests/golden/flow_stream_portscan_v1.npz, written by
    tests/golden/gen_flow_stream_portscan_golden.py): kind 8's model, the generator and the models under it have not
    moved."""
    g = np.load(GOLDEN)
    seq, par = gen_sequence(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    outs, mod = run_generated(seq, par, 8)
    assert np.array_equal(np.concatenate([o["verdict"] for o, _ in outs]), g["verdict"])
    assert np.array_equal(np.concatenate([o["acl_hit"] for o, _ in outs]), g["acl_hit"])
    assert np.array_equal(np.concatenate([o["results"] for o, _ in outs]), g["results"])
    assert np.array_equal(np.concatenate([r for _, r in outs]), g["reasons"])
    assert np.array_equal(sum(o["counters"] for o, _ in outs), g["counters"])
    assert np.array_equal(np.array(mod.cnt.c, np.uint64), g["stream_counters"])
    assert np.array_equal(np.array(mod.table(), np.uint64).reshape(-1, 10), g["flows"])
    assert np.array_equal(np.array(sorted(mod.fp.ps.records()), np.uint64).reshape(-1, 7), g["records"])
    sess = mod.sessions()
    assert np.array_equal(np.array([sum(k, ()) + sess[k] for k in sorted(sess)], np.uint64).reshape(-1, 21), g["sessions"])
    assert np.array_equal(np.array([[a[f] for f in abi.ATTACK_STATE_FIELDS] for a in mod.atk.ai], np.uint64), g["attack"])
