"""tests/flow_stream_attack_model.py against answers derived by hand from the reference (no device): where
syncount_accum takes its +1 (FlowAdd, flow.c:151-154) and its -1 (DP_Attack_SynCountFins, stream-tcp.c:608 / :660, on
the completing packet's port; StreamTcp_Flow_ResRelease, stream-tcp-session.c:61-77, on the flow's port), modulo 2^64.
Every case writes out every port's four accumulator words (udp_accum, syn_accum, syncount, syncount_accum).  Then the
state-before/after rule against the reference's own calls, packet by packet (tests/golden/ref_stream_syncount_v1.npz)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import stream_session_corpus as sc
import stream_session_model as m
from attack_model import U64, AttackModel
from conftest import GOLDEN
from flow_stream_attack_model import FlowStreamAttackModel
from pktbuild import udp_packet
from ppe import abi
from ppe.abi import ST
from stream_session_corpus import A, RS, S, c, s

NOW = 1_700_000_000
STRIDE = 144
FW = abi.ACL_RULE_ACTION_FW
Z = (0, 0, 0, 0)


def words(mod):
    return [(a["udp_accum"], a["syn_accum"], a["syncount"], a["syncount_accum"]) for a in mod.atk.ai]


def script(f, steps, cisn=1000, sisn=5000):
    return [(f, p) for p in sc.packets(steps, cisn, sisn)]


def key(f):
    cip, cport = sc.endpoints(f)
    return tuple(sorted(((cip, cport), (sc.SERVER_IP, sc.SERVER_PORT))))


@pytest.fixture
def mod():
    o = pyoracle.Oracle(np.zeros(0, abi.RULE_DTYPE), default_action=FW)
    x = FlowStreamAttackModel(o, 64, AttackModel())
    x.atk.clock(NOW)
    yield x
    x.close()


def run(mod, items, ports, now=NOW, syn_check=1, hdr=None):
    h, ln = sc.batch(items, STRIDE) if hdr is None else hdr
    out, r = mod.classify_batch(h, ln, np.array(ports, np.uint8), cfg=mod.o.cfg(0, syn_check, now))
    return (out["verdict"] & 0xFF).tolist(), r.tolist()


def test_a_handshake_completing_on_another_port(mod):
    st, r = run(mod, script(1, sc.EST), [1, 2, 2])
    assert st == [0, 0, 0] and r == [0, 0, 0] and mod.ssn[key(1)].state == m.TCP_ESTABLISHED
    # port 1: the SYN (syn_accum, +1); port 2: the SYN|ACK (syn_accum), the ACK's -1 with nothing to take it from
    assert words(mod) == [Z, (0, 1, 0, 1), (0, 1, 0, U64), Z]
    info = abi.AttackInfo()
    info.ai[2].syncount_accum = mod.atk.ai[2]["syncount_accum"]
    lib = abi.load()
    n = lib.ppe_format_attack_stat(C.byref(info), None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.ppe_format_attack_stat(C.byref(info), buf, n + 1)
    assert buf.value.decode().count("syncount_accum: -1\n") == 1  # %ld, dp_cmd.c:2518
    mod.atk.tick(NOW + 1)
    assert words(mod) == [Z, (0, 0, 1, 0), (0, 0, U64, 0), Z]
    for k, syn_count in enumerate((0xFFFFFFFF, 5, 0)):  # syncount > syn_count (dp_attack.c:673) whatever the rule holds
        mod.atk.set(td={2: dict(drop_pack=1, syn_count=syn_count)})
        st, _ = run(mod, script(2 + k, sc.SYN_SENT), [2], now=NOW + 1)
        assert st == [ST["ATTACK_SYNCOUNT"]]
    assert words(mod) == [Z, (0, 0, 1, 0), (0, 3, U64, 0), Z] and mod.atk.totals["syncount_drop"] == 3


def test_b_the_4whs_completion_decrements_on_its_packets_port(mod):
    st, r = run(mod, script(1, sc.WHS4_RECV + [s(A, 1, 1, win=3000)]), [0, 1, 2, 3])
    assert st == [0] * 4 and r == [0] * 4 and mod.ssn[key(1)].state == m.TCP_ESTABLISHED
    assert mod.ssn[key(1)].flags & m.F_4WHS
    # three packets carry SYN (ports 0, 1, 2); the to-client ACK on port 3 completes (stream-tcp.c:582-617)
    assert words(mod) == [(0, 1, 0, 1), (0, 1, 0, 0), (0, 1, 0, 0), (0, 0, 0, U64)]


def test_c_a_completing_ack_with_a_wrong_acknowledgement(mod):
    st, r = run(mod, script(1, sc.SYN_RECV + [c(A, 1, 2)]), [1, 1, 1])
    assert st == [0, 0, 29] and r[2] == m.R["WHS3_RIGHT_SEQ_WRONG_ACK_EVASION"]
    assert mod.ssn[key(1)].state == m.TCP_SYN_RECV
    assert words(mod) == [Z, (0, 2, 0, 1), Z, Z]


def test_d_aging_releases_on_the_creators_port(mod):
    items = (script(1, sc.SYN_SENT) + script(2, sc.SYN_RECV) + script(3, sc.EST) +
             script(4, sc.SYN_SENT + [s(RS | A, 0, 1)]) + script(6, [c(A, 1, 1)]))
    ports = [1] + [2, 2] + [3, 3, 3] + [0, 0] + [2]
    h, ln = sc.batch(items, STRIDE)
    u = np.frombuffer(udp_packet(0x0A0A0001, sc.SERVER_IP, 999, 53), np.uint8)
    h = np.vstack([h, np.zeros((1, STRIDE), np.uint8)])
    h[-1, :len(u)] = u
    ln = np.append(ln, np.uint32(len(u)))
    st, r = run(mod, None, ports + [1], syn_check=0, hdr=(h, ln))
    assert st == [0] + [0, 0] + [0, 0, 0] + [0, 0] + [23] + [0] and r[8] == m.R["MIDSTREAM_DISABLE"]
    assert [mod.ssn[key(f)].state for f in (1, 2, 3, 4, 6)] == [m.TCP_SYN_SENT, m.TCP_SYN_RECV, m.TCP_ESTABLISHED,
                                                                 m.TCP_CLOSED, m.TCP_NONE]
    assert mod.port == {key(1): 1, key(2): 2, key(3): 3, key(4): 0, key(6): 2}
    # port 0: flow 4's SYN; port 1: flow 1's SYN and the UDP packet; port 2: flow 2's SYN and SYN|ACK (flow 6's ACK
    # reaches no monitor and is no SYN); port 3: flow 3's SYN, SYN|ACK, and the -1 of its ACK
    assert words(mod) == [(0, 1, 0, 1), (1, 1, 0, 1), (0, 2, 0, 1), (0, 2, 0, 0)]
    assert mod.age(NOW + 100, 20) == 6
    # -1 for SYN_SENT (port 1) and SYN_RECV (port 2); none for established, closed by RST, UDP, no session
    assert words(mod) == [(0, 1, 0, 1), (1, 1, 0, 0), (0, 2, 0, 0), (0, 2, 0, 0)]
    assert mod.age(NOW + 200, 20) == 0
    assert words(mod) == [(0, 1, 0, 1), (1, 1, 0, 0), (0, 2, 0, 0), (0, 2, 0, 0)]


def test_e_a_session_reused_from_closed(mod):
    st, r = run(mod, script(1, sc.CONV_REUSE), [1] * 7 + [2])
    assert st == [0] * 8 and mod.ssn[key(1)].state == m.TCP_ESTABLISHED
    # port 1: five packets with SYN, +1 at the creation and -1 at the first establishment; port 2: the second
    # establishment's -1, and no +1 ever (the flow was found, :3083-3131)
    assert words(mod) == [Z, (0, 5, 0, 0), (0, 0, 0, U64), Z]
    # (a SYN with a sequence number past the closed session's reuses it, :3083-3131; CONV_REUSE's own c(S, 0) does not)
    st, r = run(mod, script(2, sc.CLOSED + [c(S, 77777)]), [3, 0, 0, 0, 0], now=NOW + 1)
    assert st == [0] * 5 and mod.ssn[key(2)].state == m.TCP_SYN_SENT and mod.port[key(2)] == 3
    assert words(mod) == [(0, 2, 0, U64), (0, 5, 0, 0), (0, 0, 0, U64), (0, 1, 0, 1)]
    assert mod.age(NOW + 100, 20) == 2
    # flow 2 aged in its second handshake: -1 at the port its first SYN came in on; flow 1 is established: none
    assert words(mod) == [(0, 2, 0, U64), (0, 5, 0, 0), (0, 0, 0, U64), (0, 1, 0, 0)]


def test_f_a_monitor_dropped_synack_leaves_the_session_in_syn_sent(mod):
    run(mod, script(9, sc.SYN_SENT), [2])
    mod.atk.tick(NOW + 1)
    assert words(mod) == [Z, Z, (0, 0, 1, 0), Z] and mod.atk.ai[2]["synpps"] == 1
    mod.atk.set(td={2: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)})
    st, r = run(mod, script(1, sc.EST), [1, 2, 1], now=NOW + 1)
    assert st[:2] == [0, ST["ATTACK_SYNFLOOD"]] and mod.ssn[key(1)].state == m.TCP_SYN_SENT
    assert st[2] != 0 and r[2] != 0  # the ACK meets SYN_SENT: dropped, and it establishes nothing
    assert mod.atk.ai[2]["syn_flood_hold"] == 1
    assert words(mod) == [Z, (0, 1, 0, 1), (0, 1, 1, 0), Z]


def test_the_rule_against_the_references_own_calls():
    """The reference's StreamTcpPacket over the generated conversations with DP_Attack_SynCountFins recorded
    (tests/golden/gen_stream_syncount_golden.py): it is called exactly by the steps that take SYN_RECV to ESTABLISHED."""
    g, pk = np.load(GOLDEN / "ref_stream_syncount_v1.npz"), np.load(GOLDEN / "ref_stream_session_v1.npz")
    total, calls, cnt = 0, {}, m.Counters()
    for name in ("known", "sweep", "generated"):
        if name == "generated":
            seq = sc.generate()
        else:
            seq = [(int(w[0]), m.Pkt(bool(w[7]), int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]),
                                     None if w[6] == 0xFF else int(w[6]))) for w in pk[f"{name}_pkt"]]
        fins = g[f"{name}_fins"]
        assert len(seq) == len(fins) and np.array_equal(g[f"{name}_ret"], pk[f"{name}_ret"])  # (the same run)
        assert fins.max() == 1  # never twice on one packet
        ssn = {}
        for i, (f, p) in enumerate(seq):
            x = ssn.setdefault(f, m.Session())
            before = x.state
            r = m.step(x, p, cnt)
            est = before == m.TCP_SYN_RECV and x.state == m.TCP_ESTABLISHED
            assert est == bool(fins[i]), (name, i, f, p)
            assert not (est and r), (name, i)  # a step that returns a reason never establishes
        total, calls[name] = total + len(seq), int(fins.sum())
    assert total == int(g["n"][0]) == 39282 and all(v > 50 for v in calls.values()), calls
