"""Serial model of the reference's TCP session state machine (StreamTcpPacket, dataplane/src/plugin/stream-tcp/
stream-tcp.c:2982-3143) in the one configuration the engine builds: stream_tcp_midstream 0, stream_tcp_async_oneside 0
(stream-tcp.c:20-21) and stream_tcp_reasm_enable 0, under which StreamTcpReassembleHandleSegment returns OK at once
(stream-tcp-reassemble.c:460-464) and the result is OK or ERR.  Written from the reference, line by line; the line
numbers are stream-tcp.c's unless a file is named.  The GPU tests compare the kernel with this file and nothing else.

Left out, because they cannot be taken with both settings 0 (no branch ever sets the flags that guard them):
  StreamTcpPacketStateNone's SYN|ACK pickup :263-326 and ACK pickup :372-432 (both return before, :257-261, :366-370);
  SynRecv's STREAMTCP_FLAG_MIDSTREAM_SYNACK test :621-625, its MIDSTREAM block :651-659 and the async branch :670-710;
  SynSent's async pickup :943-982 (returns at :937-941);
  Established's MIDSTREAM_ESTABLISHED block :1008-1016, the ASYNC branches :1024-1033, :1117-1165, and the
  MIDSTREAM / ASYNC terms of every in-window test (:1058-1059, :1199-1200, :1617-1618, :1672-1673, :1991-1992,
  :2058-2059); StreamTcpPacketSwitchDir :3015-3016.
SESSION_NO_MEM cannot count (one record per flow slot, no pool) and SESSION_PARAM_ERR cannot either (ssn is never NULL
in a state function: StreamTcpPacket tests it first, :3005).

The engine's definition where the reference leaves the value open: StreamTcpNewSession sets state = TCP_NONE and
nothing else (stream-tcp-session.c:22-33), so a branch may read a field no branch has written (client.window at :835);
here a session is all zero when its flow is created, and a flow without a session is an all-zero record.
Not kept: ra_app_base_seq, ra_raw_base_seq, last_ts, last_pkt_ts, os_policy, the segment lists."""
from __future__ import annotations

from dataclasses import dataclass, field

M32 = 0xFFFFFFFF

# stream-tcp-private.h:10-24
(TCP_NONE, TCP_LISTEN, TCP_SYN_SENT, TCP_SYN_RECV, TCP_ESTABLISHED, TCP_FIN_WAIT1, TCP_FIN_WAIT2, TCP_TIME_WAIT,
 TCP_LAST_ACK, TCP_CLOSE_WAIT, TCP_CLOSING, TCP_CLOSED) = range(12)
STATE_NAMES = ("NONE", "LISTEN", "SYN_SENT", "SYN_RECV", "ESTABLISHED", "FIN_WAIT1", "FIN_WAIT2", "TIME_WAIT",
               "LAST_ACK", "CLOSE_WAIT", "CLOSING", "CLOSED")
# session flags (stream-tcp-private.h:32-62) and stream flags (:70-89) this configuration can set
F_SERVER_WSCALE, F_4WHS, F_EVASION, F_3WHS_CONFIRMED = 0x0010, 0x0080, 0x0100, 0x1000
SF_KEEPALIVE, SF_CLOSE_INITIATED = 0x0004, 0x0010
TH_FIN, TH_SYN, TH_RST, TH_PUSH, TH_ACK = 0x01, 0x02, 0x04, 0x08, 0x10
TCP_WSCALE_MAX = 14  # decode-tcp.h:66

# struct tcpstream_track_stat, dataplane/src/decode/decode-statistic.h:118-179, in order
FIELDS = (
    "SYN_ACK_COUNT", "SYN_COUNT", "RST_COUNT", "RST_BUT_NO_SESSION", "FIN_BUT_NO_SESSION",
    "MIDSTREAM_OR_ONESIDE_DISABLE", "MIDSTREAM_DISABLE", "ONESIDE_DISABLE", "SESSION_NO_MEM", "FIN_INVALID_ACK",
    "FIN_OUT_OF_WINDOW", "SESSION_PARAM_ERR", "WHS3_SYNACK_TOSERVER_SYN_RECV", "WHS3_SYNACK_SEQ_MISMATCH",
    "WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK", "WHS3_SYN_TOCLIENT_ON_SYN_RECV", "WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV",
    "WHS3_SYNACK_IN_WRONG_DIRECTION", "WHS3_ACK_IN_WRONG_DIR", "WHS3_RIGHT_SEQ_WRONG_ACK_EVASION",
    "WHS3_WRONG_SEQ_WRONG_ACK", "WHS3_ASYNC_WRONG_SEQ", "WHS3_SYNACK_WITH_WRONG_ACK", "WHS4_WRONG_SEQ",
    "WHS4_INVALID_ACK", "WHS4_SYNACK_WITH_WRONG_ACK", "WHS4_SYNACK_WITH_WRONG_SYN", "EST_INVALID_ACK",
    "EST_PKT_BEFORE_LAST_ACK", "EST_PACKET_OUT_OF_WINDOW", "EST_SYNACK_RESEND", "EST_SYNACK_TOSERVER",
    "EST_SYNACK_RESEND_WITH_DIFFERENT_ACK", "EST_SYNACK_RESEND_WITH_DIFF_SEQ", "EST_SYN_TOCLIENT",
    "EST_SYN_RESEND_DIFF_SEQ", "EST_SYN_RESEND", "PKT_RETRANSMISSION", "FIN2_FIN_WRONG_SEQ", "FIN2_INVALID_ACK",
    "FIN2_ACK_WRONG_SEQ", "FIN1_FIN_WRONG_SEQ", "FIN1_INVALID_ACK", "FIN1_ACK_WRONG_SEQ", "SHUTDOWN_SYN_RESEND",
    "CLOSEWAIT_FIN_OUT_OF_WINDOW", "CLOSING_ACK_WRONG_SEQ", "CLOSEWAIT_INVALID_ACK", "CLOSING_INVALID_ACK",
    "CLOSEWAIT_PKT_BEFORE_LAST_ACK", "CLOSEWAIT_ACK_OUT_OF_WINDOW", "LASTACK_ACK_WRONG_SEQ", "LASTACK_INVALID_ACK",
    "TIMEWAIT_ACK_WRONG_SEQ", "TIMEWAIT_INVALID_ACK", "PKT_INVALID_ACK", "PKT_BAD_WINDOW_UPDATE", "PKT_BROKEN_ACK")
R = {name: i for i, name in enumerate(FIELDS)}
# the reasons that can never be returned, and the fields that only count (they never end a packet)
UNREACHABLE = {"SESSION_NO_MEM": "one record per flow slot, no pool (stream-tcp.c:266-270, :333-337)",
               "SESSION_PARAM_ERR": "ssn is never NULL in a state function (stream-tcp.c:3005 tests it first)",
               "WHS3_ASYNC_WRONG_SEQ": "behind stream_tcp_async_oneside == 0 (stream-tcp.c:937-941 returns before :947)"}
COUNT_ONLY = ("SYN_ACK_COUNT", "SYN_COUNT", "RST_COUNT", "PKT_RETRANSMISSION", "PKT_INVALID_ACK",
              "PKT_BAD_WINDOW_UPDATE", "PKT_BROKEN_ACK")
# the verdict status of a reason: StateNone's four keep the stateless path's statuses, the rest share one
ST_TRACK_DROP = 29
NONE_STATUS = {R["RST_BUT_NO_SESSION"]: 20, R["FIN_BUT_NO_SESSION"]: 21, R["MIDSTREAM_OR_ONESIDE_DISABLE"]: 22,
               R["MIDSTREAM_DISABLE"]: 23}


def seq_lt(a, b):  # SEQ_LT .. SEQ_GEQ, stream-tcp-private.h:93-97: (int32_t)(a - b) against 0
    return ((a - b) & M32) >= 0x80000000


def seq_gt(a, b):
    return 0 < ((a - b) & M32) < 0x80000000


def seq_leq(a, b):
    return not seq_gt(a, b)


def seq_geq(a, b):
    return not seq_lt(a, b)


@dataclass
class Stream:  # TcpStream, stream-tcp-private.h:118-144 (the kept fields)
    flags: int = 0
    wscale: int = 0
    isn: int = 0
    next_seq: int = 0
    last_ack: int = 0
    next_win: int = 0
    window: int = 0

    def astuple(self):
        return (self.flags, self.wscale, self.isn, self.next_seq, self.last_ack, self.next_win, self.window)


@dataclass
class Session:  # TcpSession, stream-tcp-private.h:147-153
    state: int = TCP_NONE
    flags: int = 0
    client: Stream = field(default_factory=Stream)
    server: Stream = field(default_factory=Stream)

    def astuple(self):
        return (self.state, self.flags) + self.client.astuple() + self.server.astuple()


@dataclass(frozen=True)
class Pkt:
    """What StreamTcpPacket reads of a packet: th_flags, TCP_GET_SEQ / _ACK / _WINDOW, payload_len, tcpvars.ws (ws: the
    option's shift byte, None without the option) and the flow's direction."""
    toclient: bool
    flags: int
    seq: int
    ack: int = 0
    win: int = 0
    plen: int = 0
    ws: int | None = None

    @property
    def wscale(self):  # TCP_GET_WSCALE, decode-tcp.h:103: a shift above 14 reads as 0
        return self.ws if self.ws is not None and self.ws <= TCP_WSCALE_MAX else 0


class Counters:
    def __init__(self):
        self.c = [0] * len(FIELDS)

    def add(self, name):
        self.c[R[name]] += 1
        return R[name]


def _update_last_ack(stream, ack):  # StreamTcpUpdateLastAck :36-41
    if seq_gt(ack, stream.last_ack):
        stream.last_ack = ack


def _update_next_win(stream, win):  # StreamTcpUpdateNextWin :53-58
    win &= M32
    if seq_gt(win, stream.next_win):
        stream.next_win = win


def _validate_ack(ssn, stream, p, cnt):  # StreamTcpValidateAck :73-122; True = valid
    ack = p.ack
    if seq_gt(ack, stream.last_ack) and seq_leq(ack, stream.next_win):  # :79
        return True
    if ack == stream.last_ack:  # :84
        return True
    if seq_lt(ack, stream.last_ack):  # :90
        if stream.window != 0 and seq_lt(ack, (stream.last_ack - stream.window) & M32):  # :95
            cnt.add("PKT_INVALID_ACK")
            return False
        return True
    if ssn.state > TCP_SYN_SENT and seq_gt(ack, stream.next_win):  # :104
        cnt.add("PKT_INVALID_ACK")
        return False
    if ssn.state == TCP_SYN_SENT and p.toclient and (p.flags & TH_RST) and ack == (stream.isn + 1) & M32:  # :110-114
        return True
    cnt.add("PKT_INVALID_ACK")  # :119-121
    return False


def _is_retransmission(stream, p, cnt):  # StreamTcpPacketIsRetransmission :1434-1454
    if p.plen == 0:
        return 0
    end = (p.seq + p.plen) & M32
    if seq_leq(end, stream.last_ack):
        cnt.add("PKT_RETRANSMISSION")
        return 1
    if seq_leq(end, stream.next_seq):
        cnt.add("PKT_RETRANSMISSION")
        return 2
    return 0


def _sides(ssn, p):
    """(the sender's stream, the receiver's): toserver client / server, toclient server / client, as every branch of the
    reference picks them (e.g. :2775-2781)."""
    return (ssn.server, ssn.client) if p.toclient else (ssn.client, ssn.server)


def _close_both(ssn):
    ssn.state = TCP_CLOSED
    ssn.server.flags |= SF_CLOSE_INITIATED
    ssn.client.flags |= SF_CLOSE_INITIATED


def _rst_acks(ssn, p):
    """The RST branch of FinWait1 / FinWait2 / CloseWait / LastAck / Closing / TimeWait (e.g. :1726-1747): CLOSED, both
    CLOSE_INITIATED, last_ack of the receiver's stream from the ack and of the sender's from the seq."""
    snd, rcv = _sides(ssn, p)
    _close_both(ssn)
    _update_last_ack(rcv, p.ack)
    _update_last_ack(snd, p.seq)
    return 0


def _ack_tail(ssn, p, fix_next=True):
    """last_ack of the receiver's stream, and its next_seq when the ack runs ahead of it (e.g. :1782-1788)."""
    _, rcv = _sides(ssn, p)
    _update_last_ack(rcv, p.ack)
    if fix_next and seq_lt(rcv.next_seq, p.ack):
        rcv.next_seq = p.ack


def _handle_fin(ssn, p, cnt):  # StreamTcpHandleFin :135-232
    snd, rcv = _sides(ssn, p)
    if not _validate_ack(ssn, rcv, p, cnt):  # :142, :189
        return cnt.add("FIN_INVALID_ACK")
    if seq_lt(p.seq, snd.next_seq) or seq_gt(p.seq, (snd.last_ack + snd.window) & M32):  # :149, :195
        return cnt.add("FIN_OUT_OF_WINDOW")
    ssn.state = TCP_FIN_WAIT1 if p.toclient else TCP_CLOSE_WAIT  # :159, :205
    snd.flags |= SF_CLOSE_INITIATED
    if p.seq == snd.next_seq:  # :163, :209
        snd.next_seq = (p.seq + p.plen) & M32
    rcv.window = (p.win << rcv.wscale) & M32  # :169, :215
    _ack_tail(ssn, p)  # :171-176, :217-222
    return 0


def _state_none(ssn, p, cnt):  # StreamTcpPacketStateNone :237-441
    if p.flags & TH_RST:
        return cnt.add("RST_BUT_NO_SESSION")  # :243-248
    if p.flags & TH_FIN:
        return cnt.add("FIN_BUT_NO_SESSION")  # :249-254
    if (p.flags & (TH_SYN | TH_ACK)) == (TH_SYN | TH_ACK):
        return cnt.add("MIDSTREAM_OR_ONESIDE_DISABLE")  # :255-261
    if p.flags & TH_SYN:  # :328-363
        ssn.state = TCP_SYN_SENT
        ssn.client.isn = p.seq
        ssn.client.next_seq = (p.seq + 1) & M32
        ssn.server.window = p.win
        if p.ws is not None:
            ssn.flags |= F_SERVER_WSCALE
            ssn.server.wscale = p.wscale
        return 0
    if p.flags & TH_ACK:
        return cnt.add("MIDSTREAM_DISABLE")  # :364-370
    return 0  # :434-440


def _synack_update(ssn, p):  # StreamTcp3whsSynAckUpdate :443-503
    ssn.state = TCP_SYN_RECV
    ssn.server.isn = p.seq
    ssn.server.next_seq = (p.seq + 1) & M32
    ssn.client.window = p.win
    ssn.client.last_ack = p.ack
    ssn.server.last_ack = (ssn.server.isn + 1) & M32
    ssn.client.wscale = p.wscale if (ssn.flags & F_SERVER_WSCALE) and p.ws is not None else 0  # :474-480
    ssn.server.next_win = (ssn.server.last_ack + ssn.server.window) & M32
    ssn.client.next_win = (ssn.client.last_ack + ssn.client.window) & M32
    ssn.flags &= ~F_4WHS  # :501


def _syn_sent(ssn, p, cnt):  # StreamTcpPacketStateSynSent :735-990
    c, s = ssn.client, ssn.server
    if p.flags & TH_RST:  # :747-770
        if not p.toclient:
            if p.seq == c.isn and p.win == 0 and p.ack == (c.isn + 1) & M32:
                _close_both(ssn)
        else:
            _close_both(ssn)
    elif p.flags & TH_FIN:  # :771-773
        pass
    elif (p.flags & (TH_SYN | TH_ACK)) == (TH_SYN | TH_ACK):
        if (ssn.flags & F_4WHS) and not p.toclient:  # :776-849
            if p.ack != (s.isn + 1) & M32:
                return cnt.add("WHS4_SYNACK_WITH_WRONG_ACK")
            if p.seq != c.isn:
                return cnt.add("WHS4_SYNACK_WITH_WRONG_SYN")
            ssn.state = TCP_SYN_RECV
            c.isn = p.seq
            c.next_seq = (c.isn + 1) & M32
            s.window = p.win
            s.last_ack = p.ack
            c.last_ack = (c.isn + 1) & M32
            s.wscale = p.wscale if (ssn.flags & F_SERVER_WSCALE) and p.ws is not None else 0  # :823-827
            c.next_win = (c.last_ack + c.window) & M32  # :835 (client.window: whatever the record holds)
            s.next_win = (s.last_ack + s.window) & M32
            return 0
        if not p.toclient:
            return cnt.add("WHS3_SYNACK_IN_WRONG_DIRECTION")  # :851-855
        if p.ack != (c.isn + 1) & M32:
            return cnt.add("WHS3_SYNACK_WITH_WRONG_ACK")  # :858-864
        _synack_update(ssn, p)
    elif p.flags & TH_SYN:  # :867-932
        if p.toclient:
            ssn.flags |= F_4WHS
            s.isn = p.seq
            s.next_seq = (p.seq + 1) & M32
            s.window = p.win
            if p.ws is not None:
                ssn.flags |= F_SERVER_WSCALE
                s.wscale = p.wscale
            else:
                ssn.flags &= ~F_SERVER_WSCALE
                s.wscale = 0
    elif p.flags & TH_ACK:
        return cnt.add("ONESIDE_DISABLE")  # :937-941
    return 0


def _syn_recv(ssn, p, cnt):  # StreamTcpPacketStateSynRecv :505-732
    c, s = ssn.client, ssn.server
    if p.flags & TH_RST:  # :514-527
        _close_both(ssn)
    elif p.flags & TH_FIN:  # :528-531
        return _handle_fin(ssn, p, cnt)
    elif (p.flags & (TH_SYN | TH_ACK)) == (TH_SYN | TH_ACK):  # :532-561
        if not p.toclient:
            return cnt.add("WHS3_SYNACK_TOSERVER_SYN_RECV")
        if p.ack != c.last_ack:
            return cnt.add("WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK")
        if p.seq != s.isn:
            return cnt.add("WHS3_SYNACK_SEQ_MISMATCH")
    elif p.flags & TH_SYN:  # :562-577
        if p.toclient:
            return cnt.add("WHS3_SYN_TOCLIENT_ON_SYN_RECV")
        if p.seq != c.isn:
            return cnt.add("WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV")
    elif p.flags & TH_ACK:
        if (ssn.flags & F_4WHS) and p.toclient:  # :582-617
            if p.seq != s.next_seq:
                return cnt.add("WHS4_WRONG_SEQ")
            if not _validate_ack(ssn, c, p, cnt):
                return cnt.add("WHS4_INVALID_ACK")
            _update_last_ack(c, p.ack)
            s.next_seq = (s.next_seq + p.plen) & M32
            c.window = (p.win << c.wscale) & M32
            c.next_win = (c.last_ack + c.window) & M32
            ssn.state = TCP_ESTABLISHED
            return 0
        if p.toclient:
            return cnt.add("WHS3_ACK_IN_WRONG_DIR")  # :619-632
        if p.seq == c.next_seq and p.ack == s.next_seq:  # :639-669
            _update_last_ack(s, p.ack)
            c.next_seq = (c.next_seq + p.plen) & M32
            s.window = (p.win << s.wscale) & M32
            s.next_win = (s.last_ack + s.window) & M32
            ssn.state = TCP_ESTABLISHED
            return 0
        if p.seq == c.next_seq:  # :711-717
            ssn.flags |= F_EVASION
            return cnt.add("WHS3_RIGHT_SEQ_WRONG_ACK_EVASION")
        return cnt.add("WHS3_WRONG_SEQ_WRONG_ACK")  # :718-723
    return 0


def _established_data(ssn, p, cnt):
    """HandleEstablishedPacketToClient :994-1094 and HandleEstablishedPacketToServer :1097-1240, which are one function
    of (sender's stream, receiver's stream) once the MIDSTREAM and ASYNC branches are gone."""
    snd, rcv = _sides(ssn, p)
    if not _validate_ack(ssn, rcv, p, cnt):  # :1000, :1103
        return cnt.add("EST_INVALID_ACK")
    end = (p.seq + p.plen) & M32
    if p.plen in (0, 1) and p.seq == (snd.next_seq - 1) & M32:  # keep-alive :1019-1021, :1110-1113
        pass
    elif not seq_geq(end, snd.last_ack):  # :1023, :1115
        return cnt.add("EST_PKT_BEFORE_LAST_ACK")  # :1038, :1177
    zwp = False
    if p.plen == 1 and p.seq == snd.next_seq and snd.window == 0:  # zero window probe :1046, :1185
        zwp = True
    elif snd.next_seq == p.seq:  # :1049, :1189
        snd.next_seq = (snd.next_seq + p.plen) & M32
    if zwp:
        return 0  # :1055, :1196 (falls to the function's end)
    if seq_leq(end, snd.next_win):  # :1057, :1198
        rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        _update_next_win(rcv, rcv.last_ack + rcv.window)
        return 0
    return cnt.add("EST_PACKET_OUT_OF_WINDOW")  # :1088, :1233


def _established(ssn, p, cnt):  # StreamTcpPacketStateEstablished :1257-1432
    c, s = ssn.client, ssn.server
    if p.flags & TH_RST:  # :1265-1327
        snd, rcv = _sides(ssn, p)
        _close_both(ssn)
        if not p.toclient:  # :1277-1288
            s.next_seq = p.ack
            c.next_seq = (p.seq + p.plen) & M32
            c.window = (p.win << c.wscale) & M32
        else:  # :1305-1316
            s.next_seq = (p.seq + p.plen + 1) & M32
            c.next_seq = p.ack
            s.window = (p.win << s.wscale) & M32
        _update_last_ack(rcv, p.ack)
        _update_last_ack(snd, p.seq)
        return 0
    if p.flags & TH_FIN:  # :1328-1335
        return _handle_fin(ssn, p, cnt)
    if (p.flags & (TH_SYN | TH_ACK)) == (TH_SYN | TH_ACK):  # :1336-1380
        if not p.toclient:
            return cnt.add("EST_SYNACK_TOSERVER")
        if p.ack != c.last_ack:
            return cnt.add("EST_SYNACK_RESEND_WITH_DIFFERENT_ACK")
        if p.seq != s.isn:
            return cnt.add("EST_SYNACK_RESEND_WITH_DIFF_SEQ")
        if ssn.flags & F_3WHS_CONFIRMED:
            return cnt.add("EST_SYNACK_RESEND")
        ssn.state = TCP_SYN_RECV
        return 0
    if p.flags & TH_SYN:  # :1381-1397
        if p.toclient:
            return cnt.add("EST_SYN_TOCLIENT")
        if p.seq != c.isn:
            return cnt.add("EST_SYN_RESEND_DIFF_SEQ")
        return cnt.add("EST_SYN_RESEND")
    if p.flags & TH_ACK:  # :1398-1424
        if p.toclient:
            ssn.flags |= F_3WHS_CONFIRMED
        return _established_data(ssn, p, cnt)
    return 0


def _fin_wrong_seq(snd, p):
    return seq_lt(p.seq, snd.next_seq) or seq_gt(p.seq, (snd.last_ack + snd.window) & M32)


def _fin_wait1(ssn, p, cnt):  # StreamTcpPacketStateFinWait1 :1717-2111
    snd, rcv = _sides(ssn, p)
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :1726-1747
    if p.flags & TH_FIN:  # FIN|ACK :1748-1854 (TIME_WAIT), FIN :1855-1963 (CLOSING)
        retrans = _is_retransmission(snd, p, cnt)
        if not retrans and _fin_wrong_seq(snd, p):
            return cnt.add("FIN1_FIN_WRONG_SEQ")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("FIN1_INVALID_ACK")
        if not retrans:
            ssn.state = TCP_TIME_WAIT if p.flags & TH_ACK else TCP_CLOSING
            snd.flags |= SF_CLOSE_INITIATED
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        if snd.next_seq == p.seq:
            snd.next_seq = (snd.next_seq + p.plen) & M32
        return 0
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :1964-1969
    if p.flags & TH_ACK:  # :1970-2103
        retrans = _is_retransmission(snd, p, cnt)
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("FIN1_INVALID_ACK")
        if not retrans:
            if seq_leq((p.seq + p.plen) & M32, snd.next_win):
                if p.seq == snd.next_seq:
                    ssn.state = TCP_FIN_WAIT2
            else:
                return cnt.add("FIN1_ACK_WRONG_SEQ")
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        if snd.next_seq == p.seq:
            snd.next_seq = (snd.next_seq + p.plen) & M32
        _update_next_win(rcv, rcv.last_ack + rcv.window)
    return 0


def _fin_wait2(ssn, p, cnt):  # StreamTcpPacketStateFinWait2 :1456-1714
    snd, rcv = _sides(ssn, p)
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :1465-1486
    if p.flags & TH_FIN:  # :1487-1591
        retrans = 0
        if p.seq == (snd.next_seq - 1) & M32 and p.ack == rcv.last_ack:  # :1494, :1546
            retrans = 1
        elif _is_retransmission(snd, p, cnt):
            retrans = 1
        elif _fin_wrong_seq(snd, p):
            return cnt.add("FIN2_FIN_WRONG_SEQ")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("FIN2_INVALID_ACK")
        if not retrans:
            ssn.state = TCP_TIME_WAIT
            snd.flags |= SF_CLOSE_INITIATED
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        return 0
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :1593-1596
    if p.flags & TH_ACK:  # :1597-1707
        retrans = _is_retransmission(snd, p, cnt)
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("FIN2_INVALID_ACK")
        if not retrans:
            if not seq_leq((p.seq + p.plen) & M32, snd.next_win):
                return cnt.add("FIN2_ACK_WRONG_SEQ")
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p, fix_next=False)  # :1633, :1688: last_ack only
        if snd.next_seq == p.seq:
            snd.next_seq = (snd.next_seq + p.plen) & M32
        _update_next_win(rcv, rcv.last_ack + rcv.window)
    return 0


def _close_wait(ssn, p, cnt):  # StreamTcpPacketStateCloseWait :2113-2370
    snd, rcv = _sides(ssn, p)
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :2132-2154
    if p.flags & TH_FIN:  # :2155-2254
        retrans = _is_retransmission(snd, p, cnt)
        if not retrans and _fin_wrong_seq(snd, p):
            return cnt.add("CLOSEWAIT_FIN_OUT_OF_WINDOW")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("CLOSEWAIT_INVALID_ACK")
        if not retrans:
            if p.toclient:  # :2233-2238 (toserver: the window only, :2186-2187)
                ssn.state = TCP_LAST_ACK
                snd.flags |= SF_CLOSE_INITIATED
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        return 0
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :2255-2259
    if p.flags & TH_ACK:  # :2260-2362
        retrans = _is_retransmission(snd, p, cnt)
        if p.plen > 0 and seq_leq((p.seq + p.plen) & M32, snd.last_ack):
            return cnt.add("CLOSEWAIT_PKT_BEFORE_LAST_ACK")
        if seq_gt(p.seq, (snd.last_ack + snd.window) & M32):
            return cnt.add("CLOSEWAIT_ACK_OUT_OF_WINDOW")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("CLOSEWAIT_INVALID_ACK")
        if not retrans:
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
        if p.seq == snd.next_seq:
            snd.next_seq = (snd.next_seq + p.plen) & M32
    return 0


def _last_ack(ssn, p, cnt):  # StreamTcpPacketStateLastAck :2377-2471
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :2386-2407
    if p.flags & TH_FIN:
        return 0  # :2408-2411
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :2412-2417
    if (p.flags & TH_ACK) and not p.toclient:  # :2418-2464 (a toclient ACK: nothing)
        c, s = ssn.client, ssn.server
        retrans = _is_retransmission(c, p, cnt)
        if p.seq != c.next_seq and p.seq != (c.next_seq + 1) & M32:
            return cnt.add("LASTACK_ACK_WRONG_SEQ")
        if not _validate_ack(ssn, s, p, cnt):
            return cnt.add("LASTACK_INVALID_ACK")
        if not retrans:
            ssn.state = TCP_CLOSED
            s.window = (p.win << s.wscale) & M32
        _ack_tail(ssn, p)
    return 0


def _closing(ssn, p, cnt):  # StreamTcpPacketStateClosing :2478-2607
    snd, rcv = _sides(ssn, p)
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :2487-2508
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :2509-2512
    if p.flags & TH_ACK:  # :2513-2600
        retrans = _is_retransmission(snd, p, cnt)
        if p.seq != snd.next_seq:
            return cnt.add("CLOSING_ACK_WRONG_SEQ")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("CLOSING_INVALID_ACK")
        if not retrans:
            ssn.state = TCP_TIME_WAIT
            ssn.client.window = (p.win << ssn.client.wscale) & M32  # :2542 and :2585: the client's in both directions
        _ack_tail(ssn, p)
    return 0


def _time_wait(ssn, p, cnt):  # StreamTcpPacketStateTimeWait :2614-2752
    snd, rcv = _sides(ssn, p)
    if p.flags & TH_RST:
        return _rst_acks(ssn, p)  # :2623-2646
    if p.flags & TH_FIN:
        return 0  # :2647-2648
    if p.flags & TH_SYN:
        return cnt.add("SHUTDOWN_SYN_RESEND")  # :2649-2652
    if p.flags & TH_ACK:  # :2653-2745
        retrans = 0
        if _is_retransmission(snd, p, cnt):
            retrans = 1
        elif p.seq != snd.next_seq and p.seq != (snd.next_seq + 1) & M32:
            if p.toclient and p.plen > 0 and p.seq == snd.last_ack:  # :2706-2709, the toclient side only
                return 0
            return cnt.add("TIMEWAIT_ACK_WRONG_SEQ")
        if not _validate_ack(ssn, rcv, p, cnt):
            return cnt.add("TIMEWAIT_INVALID_ACK")
        if not retrans:
            ssn.state = TCP_CLOSED
            rcv.window = (p.win << rcv.wscale) & M32
        _ack_tail(ssn, p)
    return 0


_STATE_FN = {TCP_SYN_SENT: _syn_sent, TCP_SYN_RECV: _syn_recv, TCP_ESTABLISHED: _established,
             TCP_CLOSE_WAIT: _close_wait, TCP_FIN_WAIT1: _fin_wait1, TCP_FIN_WAIT2: _fin_wait2,
             TCP_LAST_ACK: _last_ack, TCP_CLOSING: _closing, TCP_TIME_WAIT: _time_wait}


def step(ssn: Session, p: Pkt, cnt: Counters) -> int:
    """StreamTcpPacket :2982-3143 for one packet: updates ssn and cnt, returns 0 (STREAMTCP_OK) or the index in FIELDS
    of the reason counted last (STREAMTCP_ERR)."""
    if (p.flags & (TH_SYN | TH_ACK)) == (TH_SYN | TH_ACK):  # :2989-2997
        cnt.add("SYN_ACK_COUNT")
    elif p.flags & TH_SYN:
        cnt.add("SYN_COUNT")
    if p.flags & TH_RST:
        cnt.add("RST_COUNT")
    if not (p.flags & TH_ACK) and p.ack != 0:  # :3000-3003
        cnt.add("PKT_BROKEN_ACK")
    if ssn.state == TCP_NONE:  # :3005-3008
        return _state_none(ssn, p, cnt)
    snd, rcv = _sides(ssn, p)
    sfr = p.flags & (TH_SYN | TH_FIN | TH_RST)
    # StreamTcpPacketIsKeepAlive :2804-2844
    if p.plen <= 1 and not sfr and p.ack == rcv.last_ack and p.seq == (snd.next_seq - 1) & M32:
        snd.flags |= SF_KEEPALIVE
        return 0  # :3018-3021
    pkt_win = (p.win << rcv.wscale) & M32
    # StreamTcpPacketIsKeepAliveACK :2757-2798
    if (p.plen == 0 and not sfr and p.win != 0 and pkt_win == rcv.window and (rcv.flags & SF_KEEPALIVE) and
            p.ack == rcv.last_ack and p.seq == snd.next_seq):
        rcv.flags &= ~SF_KEEPALIVE
        snd.flags &= ~SF_KEEPALIVE  # StreamTcpClearKeepAliveFlag :3024
        return 0
    snd.flags &= ~SF_KEEPALIVE  # :3029
    # StreamTcpPacketIsWindowUpdate :2864-2905, else StreamTcpPacketIsBadWindowUpdate :2923-2972
    wupdate = (ssn.state >= TCP_ESTABLISHED and p.plen == 0 and not sfr and p.win != 0 and pkt_win != rcv.window and
               p.ack == rcv.last_ack and p.seq == snd.next_seq)
    if not wupdate and ssn.state >= TCP_ESTABLISHED and not sfr and pkt_win < rcv.window:
        if rcv.window - pkt_win > p.plen and seq_gt(p.ack, rcv.next_seq) and seq_gt(p.seq, snd.next_seq):
            cnt.add("PKT_BAD_WINDOW_UPDATE")
            return 0  # :3038-3042
    if ssn.state == TCP_CLOSED:  # :3083-3131
        if not p.toclient and (p.flags & TH_SYN) and not (p.flags & TH_ACK) and p.seq != ssn.client.isn:
            ssn.state = TCP_NONE
            ssn.flags = 0
            ssn.client.flags = 0
            ssn.server.flags = 0
            return _state_none(ssn, p, cnt)
        return 0
    fn = _STATE_FN.get(ssn.state)
    return fn(ssn, p, cnt) if fn else 0  # (TCP_LISTEN: the default case :3132-3136)


def status_of(reason: int) -> int:
    """The verdict status of a dropped packet: 20-23 for StreamTcpPacketStateNone's four, PPE_ST_STREAM_TRACK_DROP else."""
    return NONE_STATUS.get(reason, ST_TRACK_DROP)
