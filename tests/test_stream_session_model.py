"""Known answers for the serial model of the TCP session machine (tests/stream_session_model.py), worked out by hand
from dataplane/src/plugin/stream-tcp/stream-tcp.c, the coverage table over struct tcpstream_track_stat, and the
generated conversations the GPU tests run.  CPU only."""
import re
from pathlib import Path

import pytest

import stream_session_corpus as sc
import stream_session_model as m
from stream_session_corpus import A, F, P, RS, S, c, run, s

ROOT = Path(__file__).resolve().parent.parent
OK = 0


def names(res):
    return [(m.FIELDS[r] if r else None, m.STATE_NAMES[st]) for r, st in res]


def last(script, **kw):
    res, ssn, cnt = run(script, **kw)
    r, st = res[-1]
    return (m.FIELDS[r] if r else None), m.STATE_NAMES[st], ssn, cnt


def test_fields_are_the_reference_struct():
    """58 names in the order of struct tcpstream_track_stat; the header's PPE_STC_* list mirrors them."""
    assert len(m.FIELDS) == 58 and len(set(m.FIELDS)) == 58
    assert m.FIELDS[0] == "SYN_ACK_COUNT" and m.FIELDS[9] == "FIN_INVALID_ACK" and m.FIELDS[57] == "PKT_BROKEN_ACK"
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    got = re.findall(r"PPE_STC_([A-Z0-9_]+)", hdr.split("enum ppe_stream_track_counter {")[1].split("}")[0])
    assert tuple(got[:58]) == m.FIELDS


def test_complete_conversation():
    """SYN, SYN|ACK, ACK, 100 B up, 200 B down, ACK, then the server's FIN, its ACK, the client's FIN, its ACK:
    FIN_WAIT1, FIN_WAIT2, TIME_WAIT, CLOSED.  A FIN takes no sequence number here (StreamTcpHandleFin :163-164 adds
    payload_len only), so the last ACKs are what move next_seq (:1787-1788, :2737-2738)."""
    res, ssn, cnt = run(sc.CONV_SERVER_CLOSES)
    assert names(res) == [(None, x) for x in ("SYN_SENT", "SYN_RECV", "ESTABLISHED", "ESTABLISHED", "ESTABLISHED",
                                              "ESTABLISHED", "FIN_WAIT1", "FIN_WAIT2", "TIME_WAIT", "CLOSED")]
    assert ssn.flags == m.F_3WHS_CONFIRMED
    #                          flags wscale isn  next_seq last_ack next_win window
    assert ssn.client.astuple() == (0x10, 0, 1000, 1102, 1102, 3101, 2000)
    assert ssn.server.astuple() == (0x10, 0, 5000, 5202, 5202, 6202, 1000)
    assert cnt.c[m.R["SYN_COUNT"]] == 1 and cnt.c[m.R["SYN_ACK_COUNT"]] == 1 and sum(cnt.c) == 2


def test_the_other_closing_paths():
    res, ssn, _ = run(sc.CONV_CLIENT_CLOSES)
    assert [x for _, x in names(res)][-4:] == ["CLOSE_WAIT", "CLOSE_WAIT", "LAST_ACK", "CLOSED"]
    assert all(r == OK for r, _ in res)
    res, ssn, cnt = run(sc.CONV_BOTH_CLOSE)
    assert [x for _, x in names(res)][-4:] == ["FIN_WAIT1", "CLOSING", "TIME_WAIT", "CLOSED"]
    assert all(r == OK for r, _ in res) and cnt.c[m.R["PKT_BROKEN_ACK"]] == 1  # the FIN without ACK carries an ack


def test_handshake_rejections():
    assert last(sc.SYN_SENT + [s(S | A, 0, 2)])[:2] == ("WHS3_SYNACK_WITH_WRONG_ACK", "SYN_SENT")
    assert last(sc.SYN_SENT + [c(S | A, 0, 1)])[:2] == ("WHS3_SYNACK_IN_WRONG_DIRECTION", "SYN_SENT")
    assert last(sc.SYN_RECV + [c(S | A, 0, 1)])[:2] == ("WHS3_SYNACK_TOSERVER_SYN_RECV", "SYN_RECV")
    assert last(sc.EST + [c(S | A, 0, 1)])[:2] == ("EST_SYNACK_TOSERVER", "ESTABLISHED")
    r, st, ssn, _ = last(sc.SYN_RECV + [c(A, 1, 2)])  # the evasion attempt of :711-716
    assert (r, st, ssn.flags) == ("WHS3_RIGHT_SEQ_WRONG_ACK_EVASION", "SYN_RECV", m.F_EVASION)
    assert last(sc.SYN_RECV + [c(A, 2, 2)])[:2] == ("WHS3_WRONG_SEQ_WRONG_ACK", "SYN_RECV")
    assert last(sc.SYN_RECV + [s(A, 1, 1)])[:2] == ("WHS3_ACK_IN_WRONG_DIR", "SYN_RECV")
    assert last(sc.SYN_SENT + [c(A, 1, 1)])[:2] == ("ONESIDE_DISABLE", "SYN_SENT")
    # seq = next_seq - 1 with the right ack is a keep-alive before it is a handshake ACK (:3018 runs first)
    r, st, ssn, _ = last(sc.SYN_RECV + [c(A, 0, 1)])
    assert (r, st, ssn.client.flags) == (None, "SYN_RECV", m.SF_KEEPALIVE)


def test_four_way_handshake():
    res, ssn, _ = run(sc.CONV_4WHS[:4])
    assert names(res) == [(None, "SYN_SENT"), (None, "SYN_SENT"), (None, "SYN_RECV"), (None, "ESTABLISHED")]
    assert ssn.flags == m.F_4WHS  # only StreamTcp3whsSynAckUpdate clears it (:501)
    # client.window is read at :835 before anything wrote it: the zero record makes next_win = last_ack
    assert ssn.client.astuple() == (0, 0, 1000, 1001, 1001, 4001, 3000)
    assert ssn.server.astuple() == (0, 0, 5000, 5001, 5001, 6501, 1500)
    assert last(sc.WHS4_SENT + [c(S | A, 0, 2)])[:2] == ("WHS4_SYNACK_WITH_WRONG_ACK", "SYN_SENT")
    assert last(sc.WHS4_SENT + [c(S | A, 1, 1)])[:2] == ("WHS4_SYNACK_WITH_WRONG_SYN", "SYN_SENT")
    assert last(sc.WHS4_RECV + [s(A, 2, 1)])[:2] == ("WHS4_WRONG_SEQ", "SYN_RECV")
    r, st, _, cnt = last(sc.WHS4_RECV + [s(A, 1, 500)])
    assert (r, st, cnt.c[m.R["PKT_INVALID_ACK"]]) == ("WHS4_INVALID_ACK", "SYN_RECV", 1)


@pytest.mark.parametrize("pre,state", sc.PREFIX_STATE, ids=lambda x: None)
def test_rst_in_each_state(pre, state):
    assert run(pre)[0][-1] == (OK, state)
    for pkt in (c(RS | A, 1, 1), s(RS | A, 1, 1)):
        r, st, ssn, cnt = last(pre + [pkt])
        if state == m.TCP_SYN_SENT and pkt[0] == "c":  # :753-762: only seq = isn, window 0, ack = isn + 1 resets
            assert (r, st) == (None, "SYN_SENT")
        else:
            assert (r, st) == (None, "CLOSED")
            if state != m.TCP_CLOSED:
                assert ssn.client.flags & ssn.server.flags & m.SF_CLOSE_INITIATED
        assert cnt.c[m.R["RST_COUNT"]] == (2 if state == m.TCP_CLOSED else 1)
    # without a session: RST_BUT_NO_SESSION
    assert last([c(RS | S, 0)])[:2] == ("RST_BUT_NO_SESSION", "NONE")


def test_rst_to_server_in_syn_sent_needs_the_exact_numbers():
    rst = m.Pkt(False, RS | A, 1000, 1001, 0)
    ssn, cnt = m.Session(), m.Counters()
    assert m.step(ssn, m.Pkt(False, S, 1000, 0, 1000), cnt) == OK
    assert m.step(ssn, m.Pkt(False, RS | A, 1000, 1001, 5), cnt) == OK and ssn.state == m.TCP_SYN_SENT
    assert m.step(ssn, rst, cnt) == OK and ssn.state == m.TCP_CLOSED


def test_syn_resent():
    assert last(sc.SYN_RECV + [c(S, 0)])[:2] == (None, "SYN_RECV")
    assert last(sc.SYN_RECV + [c(S, 5)])[:2] == ("WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV", "SYN_RECV")
    assert last(sc.EST + [c(S, 0)])[:2] == ("EST_SYN_RESEND", "ESTABLISHED")
    assert last(sc.EST + [c(S, 5)])[:2] == ("EST_SYN_RESEND_DIFF_SEQ", "ESTABLISHED")
    for pre in sc.SHUTDOWN_STATES:
        assert last(pre + [c(S, 0)])[0] == "SHUTDOWN_SYN_RESEND"
    # a SYN|ACK resent before the server's first ACK takes the session back to SYN_RECV (:1365-1379)
    assert last(sc.EST + [s(S | A, 0, 1)])[:2] == (None, "SYN_RECV")
    assert last(sc.EST + [s(A, 1, 1), s(S | A, 0, 1)])[:2] == ("EST_SYNACK_RESEND", "ESTABLISHED")


def test_window_edges():
    before = sc.EST + [c(A | P, 1, 1, plen=100), s(A, 1, 101)]
    assert last(before + [c(A | P, 1, 1, plen=50)])[:2] == ("EST_PKT_BEFORE_LAST_ACK", "ESTABLISHED")
    assert last(before + [c(A | P, 1, 1, plen=100)])[0] is None  # ends at last_ack: SEQ_GEQ holds (:1115)
    r, _, ssn, _ = last(sc.EST + [c(A | P, 1, 1, plen=sc.SW)])  # ends at next_win = 1001 + 2000
    assert r is None and ssn.client.next_seq == 3001
    r, _, ssn, _ = last(sc.EST + [c(A | P, 1, 1, plen=sc.SW + 1)])
    assert r == "EST_PACKET_OUT_OF_WINDOW" and ssn.client.next_seq == 3002  # next_seq moved before the test (:1189)
    # zero window: the server advertised 0, one byte at next_seq is a probe and skips the window test (:1185, :1196)
    zero = sc.SYN_SENT + [s(S | A, 0, 1, win=0), c(A, 1, 1)]
    r, _, ssn, _ = last(zero + [c(A | P, 1, 1, plen=1)])
    assert r is None and ssn.client.next_seq == 1001
    assert last(zero + [c(A | P, 1, 1, plen=2)])[0] == "EST_PACKET_OUT_OF_WINDOW"


def test_keepalive_and_window_updates():
    res, ssn, cnt = run(sc.EST + [c(A, 0, 1)])
    assert res[-1] == (OK, m.TCP_ESTABLISHED) and ssn.client.flags == m.SF_KEEPALIVE
    res, ssn, cnt = run(sc.EST + [c(A, 0, 1), s(A, 1, 1)])
    # the keep-alive ACK returns before the state function: no 3WHS_CONFIRMED, flag cleared (:2792, :3024)
    assert res[-1] == (OK, m.TCP_ESTABLISHED) and ssn.client.flags == 0 and ssn.flags == 0
    r, _, ssn, _ = last(sc.EST + [s(A, 1, 1, win=4000)])  # a window update goes on to the state function
    assert r is None and ssn.client.window == 4000 and ssn.client.next_win == 5001 and ssn.flags == m.F_3WHS_CONFIRMED
    r, _, ssn, cnt = last(sc.EST + [s(A, 101, 201, win=500)])  # shrinks by 1500, acks and sends unseen data
    assert r is None and cnt.c[m.R["PKT_BAD_WINDOW_UPDATE"]] == 1 and ssn.client.window == 2000 and ssn.flags == 0


def test_retransmission_in_last_ack():
    r, st, _, cnt = last(sc.LAST_ACK + [c(A | P, -99, 1, plen=100)])
    assert (r, st, cnt.c[m.R["PKT_RETRANSMISSION"]]) == ("LASTACK_ACK_WRONG_SEQ", "LAST_ACK", 1)
    assert last(sc.LAST_ACK + [c(A, 1, 2)])[:2] == (None, "CLOSED")
    assert last(sc.LAST_ACK + [s(A, 1, 1)])[:2] == (None, "LAST_ACK")  # a toclient ACK: nothing (:2420)


def test_reuse_of_a_closed_session():
    res, ssn, _ = run(sc.CONV_REUSE)
    assert names(res)[-4:] == [(None, "CLOSED"), (None, "SYN_SENT"), (None, "SYN_RECV"), (None, "ESTABLISHED")]
    assert ssn.client.isn == 1000 + 77777 and ssn.client.flags == 0 and ssn.flags == 0
    r, st, ssn, _ = last(sc.CLOSED + [s(S, 0)])  # to the client: no reuse
    assert (r, st) == (None, "CLOSED")


def test_window_scale_on_one_side_only():
    r, _, ssn, _ = last([c(S, 0, ws=7), s(S | A, 0, 1), c(A, 1, 1, win=10)])
    assert (ssn.flags, ssn.server.wscale, ssn.client.wscale, ssn.server.window) == (m.F_SERVER_WSCALE, 7, 0, 1280)
    assert ssn.server.next_win == 5001 + 1280
    r, _, ssn, _ = last([c(S, 0), s(S | A, 0, 1, ws=5), c(A, 1, 1, win=10)])
    assert (ssn.flags, ssn.server.wscale, ssn.client.wscale, ssn.server.window) == (0, 0, 0, 10)
    r, _, ssn, _ = last([c(S, 0, ws=7), s(S | A, 0, 1, ws=5), c(A, 1, 1, win=10)])
    assert (ssn.server.wscale, ssn.client.wscale) == (7, 5)
    r, _, ssn, _ = last([c(S, 0, ws=15), s(S | A, 0, 1, ws=14), c(A, 1, 1, win=10)])  # above 14 reads as 0
    assert (ssn.flags, ssn.server.wscale, ssn.client.wscale) == (m.F_SERVER_WSCALE, 0, 14)


def test_sequence_numbers_that_wrap():
    res, ssn, _ = run(sc.EST + [c(A | P, 1, 1, plen=100)], cisn=0xFFFFFFF0, sisn=0xFFFFFFFF)
    assert all(r == OK for r, _ in res) and ssn.state == m.TCP_ESTABLISHED
    assert (ssn.server.isn, ssn.server.next_seq, ssn.server.last_ack) == (0xFFFFFFFF, 0, 0)
    assert (ssn.client.next_seq, ssn.client.next_win) == (0x55, (0xFFFFFFF1 + 2000) & m.M32)
    for cisn, sisn in sc.ISNS:
        for conv in sc.CONVERSATIONS:
            assert [r for r, _ in run(conv, cisn, sisn)[0]] == [r for r, _ in run(conv)[0]]


# every field: the trigger that produces it, or why nothing can
COVERAGE = {f: ("trigger", pre, steps) for f, pre, steps in sc.TRIGGERS}
COVERAGE.update({f: ("unreachable", why) for f, why in m.UNREACHABLE.items()})


def test_coverage_table_has_every_field():
    assert set(COVERAGE) == set(m.FIELDS) and len(COVERAGE) == 58


@pytest.mark.parametrize("name", [f for f in m.FIELDS if f not in m.UNREACHABLE])
def test_every_reachable_field_has_a_known_answer(name):
    _, pre, steps = COVERAGE[name]
    res, _, cnt = run(pre + steps)
    assert all(r == OK for r, _ in res[:-1]), names(res)
    if name in m.COUNT_ONLY:
        assert cnt.c[m.R[name]] >= 1
    else:
        assert res[-1][0] == m.R[name] >= 9 or name in ("RST_BUT_NO_SESSION", "FIN_BUT_NO_SESSION",
                                                        "MIDSTREAM_OR_ONESIDE_DISABLE", "MIDSTREAM_DISABLE",
                                                        "ONESIDE_DISABLE") and res[-1][0] == m.R[name]
        assert cnt.c[m.R[name]] == 1
        assert m.status_of(res[-1][0]) == (20 + m.R[name] - 3 if 3 <= m.R[name] <= 6 else 29)


def test_generated_conversations_reach_everything():
    seq = sc.generate()
    assert 2000 < len(seq) < 6000
    reasons, ssn, cnt = sc.model_run(seq)
    seen = set()
    # replay per flow to see the states passed through
    per = {}
    for f, p in seq:
        per.setdefault(f, []).append(p)
    for f, pk in per.items():
        x, k = m.Session(), m.Counters()
        for p in pk:
            m.step(x, p, k)
            seen.add(x.state)
        assert x.astuple() == ssn[f].astuple()
    assert seen >= {m.TCP_SYN_SENT, m.TCP_SYN_RECV, m.TCP_ESTABLISHED, m.TCP_FIN_WAIT1, m.TCP_FIN_WAIT2,
                    m.TCP_TIME_WAIT, m.TCP_LAST_ACK, m.TCP_CLOSE_WAIT, m.TCP_CLOSING, m.TCP_CLOSED}
    for name in m.FIELDS:
        if name in m.UNREACHABLE:
            assert cnt.c[m.R[name]] == 0
        elif name in m.COUNT_ONLY:
            assert cnt.c[m.R[name]] >= 10, name
        else:
            assert reasons.count(m.R[name]) >= 10, (name, reasons.count(m.R[name]))
            assert cnt.c[m.R[name]] == reasons.count(m.R[name])


# ---- the pin by the reference itself: tests/golden/ref_stream_session_v1.npz, the reference's own stream-tcp.c compiled
# against stand-in headers and run over these sequences (tests/golden/gen_stream_session_golden.py)

def _reference_sequences():
    import numpy as np
    from conftest import GOLDEN
    g = np.load(GOLDEN / "ref_stream_session_v1.npz")
    for name in ("known", "sweep", "generated"):
        if name == "generated":
            seq = sc.generate()
        else:
            seq = [(int(w[0]), m.Pkt(bool(w[7]), int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]),
                                     None if w[6] == 0xFF else int(w[6]))) for w in g[f"{name}_pkt"]]
        assert len(seq) == int(g[f"{name}_n"][0])
        yield name, seq, g[f"{name}_ret"], g[f"{name}_changed"], g[f"{name}_counters"], g[f"{name}_sessions"]


def test_model_equals_the_reference_packet_by_packet():
    """Every packet's OK / ERR, the fields of tcpstream_track_stat it changed, the counters at the end and every flow's
    final session are the reference's own; the reason the model returns is the one changed field that is neither a
    count-first nor a count-only field."""
    total = 0
    for name, seq, ret, changed, counters, sessions in _reference_sequences():
        ssn, cnt = {}, m.Counters()
        for i, (f, p) in enumerate(seq):
            before = list(cnt.c)
            r = m.step(ssn.setdefault(f, m.Session()), p, cnt)
            assert (r != 0) == bool(ret[i]), (name, i, p, r)
            delta = [k for k in range(58) if cnt.c[k] != before[k]][:4]
            want = [(int(changed[i]) >> (8 * k)) & 0xFF for k in range(4)]
            assert delta == [x for x in want if x != 0xFF], (name, i, p, delta, want)
            if r:
                assert cnt.c[r] == before[r] + 1 and m.FIELDS[r] not in m.COUNT_ONLY
        assert cnt.c == counters.tolist(), name
        for f in range(len(sessions)):
            assert ssn.get(f, m.Session()).astuple() == tuple(int(x) for x in sessions[f]), (name, f)
        total += len(seq)
    assert total > 35000
