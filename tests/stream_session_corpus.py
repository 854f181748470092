"""Conversations for the TCP session machine (tests/stream_session_model.py): scripts written relative to the two
initial sequence numbers, the directed triggers of every reachable field of tcpstream_track_stat, whole conversations
down every closing path, a seeded generator that mixes them over many flows, and the frames that carry them.

A script is a list of steps (side, th_flags, dseq, dack, win, plen, ws): side 'c' is the flow's creator (toserver),
's' the other end (toclient); seq = own ISN + dseq, ack = peer's ISN + dack (dack None: 0)."""
from __future__ import annotations

import struct

import numpy as np

import stream_session_model as m
from stream_session_model import TH_ACK as A, TH_FIN as F, TH_PUSH as P, TH_RST as RS, TH_SYN as S

CW, SW = 1000, 2000  # the windows the client / the server advertise unless a step says otherwise


def c(flags, dseq, dack=None, win=CW, plen=0, ws=None):
    return ("c", flags, dseq, dack, win, plen, ws)


def s(flags, dseq, dack=None, win=SW, plen=0, ws=None):
    return ("s", flags, dseq, dack, win, plen, ws)


def packets(script, cisn, sisn):
    """The script's steps as model packets for the two ISNs."""
    out = []
    for side, flags, dseq, dack, win, plen, ws in script:
        own, peer = (cisn, sisn) if side == "c" else (sisn, cisn)
        out.append(m.Pkt(side == "s", flags, (own + dseq) & m.M32, 0 if dack is None else (peer + dack) & m.M32, win,
                         plen, ws))
    return out


# ---- the way into every state (ISNs C and S; after the handshake client.next_win = C+1+SW, server.next_win = S+1+CW)
SYN_SENT = [c(S, 0)]
SYN_RECV = SYN_SENT + [s(S | A, 0, 1)]
EST = SYN_RECV + [c(A, 1, 1)]
FIN_WAIT1 = EST + [s(F | A, 1, 1)]             # the server closes first (StreamTcpHandleFin toclient)
FIN_WAIT2 = FIN_WAIT1 + [c(A, 1, 2)]
TIME_WAIT = FIN_WAIT2 + [c(F | A, 1, 2)]
CLOSING = FIN_WAIT1 + [c(F, 1, 1)]              # a FIN without ACK (FinWait1's second FIN branch)
CLOSE_WAIT = EST + [c(F | A, 1, 1)]            # the client closes first
LAST_ACK = CLOSE_WAIT + [s(F | A, 1, 1)]
CLOSED = EST + [c(RS | A, 1, 1)]
WHS4_SENT = SYN_SENT + [s(S, 0, win=3000)]      # SYN in the opposite direction: STREAMTCP_FLAG_4WHS
WHS4_RECV = WHS4_SENT + [c(S | A, 0, 1, win=1500)]
PREFIX_STATE = [(SYN_SENT, m.TCP_SYN_SENT), (SYN_RECV, m.TCP_SYN_RECV), (EST, m.TCP_ESTABLISHED),
                (FIN_WAIT1, m.TCP_FIN_WAIT1), (FIN_WAIT2, m.TCP_FIN_WAIT2), (TIME_WAIT, m.TCP_TIME_WAIT),
                (CLOSING, m.TCP_CLOSING), (CLOSE_WAIT, m.TCP_CLOSE_WAIT), (LAST_ACK, m.TCP_LAST_ACK),
                (CLOSED, m.TCP_CLOSED), (WHS4_SENT, m.TCP_SYN_SENT), (WHS4_RECV, m.TCP_SYN_RECV)]

FAR = 4000  # an acknowledgement this far past the peer's ISN lies beyond every next_win above

# ---- one directed trigger per reachable field: (field, the way in, the steps whose last one produces it).  For a
# reason the last step is dropped with it; for a count-only field the last step counts it.
TRIGGERS = [
    ("SYN_ACK_COUNT", SYN_SENT, [s(S | A, 0, 1)]),
    ("SYN_COUNT", [], [c(S, 0)]),
    ("RST_COUNT", EST, [c(RS | A, 1, 1)]),
    ("RST_BUT_NO_SESSION", [], [c(RS | S, 0)]),
    ("FIN_BUT_NO_SESSION", [], [c(F | S, 0)]),
    ("MIDSTREAM_OR_ONESIDE_DISABLE", [], [c(S | A, 0, 1)]),
    ("MIDSTREAM_DISABLE", [], [c(A, 0, 1)]),
    ("ONESIDE_DISABLE", SYN_SENT, [c(A, 1, 1)]),
    ("FIN_INVALID_ACK", EST, [c(F | A, 1, FAR)]),
    ("FIN_OUT_OF_WINDOW", EST, [c(F | A, -100, 1)]),
    ("WHS3_SYNACK_TOSERVER_SYN_RECV", SYN_RECV, [c(S | A, 0, 1)]),
    ("WHS3_SYNACK_SEQ_MISMATCH", SYN_RECV, [s(S | A, 5, 1)]),
    ("WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK", SYN_RECV, [s(S | A, 0, 5)]),
    ("WHS3_SYN_TOCLIENT_ON_SYN_RECV", SYN_RECV, [s(S, 0)]),
    ("WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV", SYN_RECV, [c(S, 5)]),
    ("WHS3_SYNACK_IN_WRONG_DIRECTION", SYN_SENT, [c(S | A, 0, 1)]),
    ("WHS3_ACK_IN_WRONG_DIR", SYN_RECV, [s(A, 1, 1)]),
    ("WHS3_RIGHT_SEQ_WRONG_ACK_EVASION", SYN_RECV, [c(A, 1, 2)]),
    ("WHS3_WRONG_SEQ_WRONG_ACK", SYN_RECV, [c(A, 2, 2)]),
    ("WHS3_SYNACK_WITH_WRONG_ACK", SYN_SENT, [s(S | A, 0, 2)]),
    ("WHS4_WRONG_SEQ", WHS4_RECV, [s(A, 2, 1, win=3000)]),
    ("WHS4_INVALID_ACK", WHS4_RECV, [s(A, 1, 500, win=3000)]),
    ("WHS4_SYNACK_WITH_WRONG_ACK", WHS4_SENT, [c(S | A, 0, 2)]),
    ("WHS4_SYNACK_WITH_WRONG_SYN", WHS4_SENT, [c(S | A, 1, 1)]),
    ("EST_INVALID_ACK", EST, [c(A, 1, FAR)]),
    ("EST_PKT_BEFORE_LAST_ACK", EST, [c(A | P, 1, 1, plen=100), s(A, 1, 101), c(A | P, 1, 1, plen=50)]),
    ("EST_PACKET_OUT_OF_WINDOW", EST, [c(A | P, 1, 1, plen=SW + 1)]),
    ("EST_SYNACK_RESEND", EST, [s(A, 1, 1), s(S | A, 0, 1)]),
    ("EST_SYNACK_TOSERVER", EST, [c(S | A, 0, 1)]),
    ("EST_SYNACK_RESEND_WITH_DIFFERENT_ACK", EST, [s(S | A, 0, 9)]),
    ("EST_SYNACK_RESEND_WITH_DIFF_SEQ", EST, [s(S | A, 9, 1)]),
    ("EST_SYN_TOCLIENT", EST, [s(S, 0)]),
    ("EST_SYN_RESEND_DIFF_SEQ", EST, [c(S, 9)]),
    ("EST_SYN_RESEND", EST, [c(S, 0)]),
    ("PKT_RETRANSMISSION", LAST_ACK, [c(A | P, -99, 1, plen=100)]),
    ("FIN2_FIN_WRONG_SEQ", FIN_WAIT2, [c(F | A, -100, 2)]),
    ("FIN2_INVALID_ACK", FIN_WAIT2, [c(A, 1, FAR)]),
    ("FIN2_ACK_WRONG_SEQ", FIN_WAIT2, [c(A | P, 1, 2, plen=SW + 500)]),
    ("FIN1_FIN_WRONG_SEQ", FIN_WAIT1, [c(F | A, -100, 1)]),
    ("FIN1_INVALID_ACK", FIN_WAIT1, [c(A, 1, FAR)]),
    ("FIN1_ACK_WRONG_SEQ", FIN_WAIT1, [c(A | P, 1, 1, plen=SW + 500)]),
    ("SHUTDOWN_SYN_RESEND", FIN_WAIT1, [c(S, 0)]),
    ("CLOSEWAIT_FIN_OUT_OF_WINDOW", CLOSE_WAIT, [s(F | A, -1000, 1)]),
    ("CLOSING_ACK_WRONG_SEQ", CLOSING, [s(A, 5, 1)]),
    ("CLOSEWAIT_INVALID_ACK", CLOSE_WAIT, [s(A, 1, FAR)]),
    ("CLOSING_INVALID_ACK", CLOSING, [s(A, 1, FAR)]),
    ("CLOSEWAIT_PKT_BEFORE_LAST_ACK", CLOSE_WAIT, [s(A | P, -100, 1, plen=50)]),
    ("CLOSEWAIT_ACK_OUT_OF_WINDOW", CLOSE_WAIT, [s(A, 1 + CW + 1000, 1)]),
    ("LASTACK_ACK_WRONG_SEQ", LAST_ACK, [c(A, 5, 1)]),
    ("LASTACK_INVALID_ACK", LAST_ACK, [c(A, 1, FAR)]),
    ("TIMEWAIT_ACK_WRONG_SEQ", TIME_WAIT, [s(A, 9, 1)]),
    ("TIMEWAIT_INVALID_ACK", TIME_WAIT, [s(A, 2, FAR)]),
    ("PKT_INVALID_ACK", EST, [c(A, 1, FAR)]),
    ("PKT_BAD_WINDOW_UPDATE", EST, [s(A, 101, 201, win=500)]),
    ("PKT_BROKEN_ACK", [], [c(S, 0, 5)]),
]
# SYN resent in every shutdown state, for SHUTDOWN_SYN_RESEND's six callers
SHUTDOWN_STATES = [FIN_WAIT1, FIN_WAIT2, TIME_WAIT, CLOSING, CLOSE_WAIT, LAST_ACK]

# ---- whole conversations
DATA = [c(A | P, 1, 1, plen=100), s(A | P, 1, 101, plen=200), c(A, 101, 201)]
CONV_SERVER_CLOSES = EST + DATA + [s(F | A, 201, 101), c(A, 101, 202), c(F | A, 101, 202), s(A, 202, 102)]
CONV_CLIENT_CLOSES = EST + DATA + [c(F | A, 101, 201), s(A, 201, 102), s(F | A, 201, 102), c(A, 102, 202)]
CONV_BOTH_CLOSE = EST + DATA + [s(F | A, 201, 101), c(F, 101, 201), s(A, 201, 101), s(A, 201, 102)]
CONV_4WHS = WHS4_RECV + [s(A, 1, 1, win=3000), c(A | P, 1, 1, plen=10), s(A, 1, 11, win=3000)]
CONV_KEEPALIVE = EST + [c(A, 0, 1), s(A, 1, 1), s(A, 1, 1, win=4000), c(RS | A, 1, 1)]
CONV_WSCALE = [c(S, 0, ws=7), s(S | A, 0, 1, ws=5), c(A, 1, 1, win=10), c(A | P, 1, 1, win=10, plen=1000),
               s(A, 1, 1001, win=100)]
CONV_REUSE = CLOSED + [c(S, 0), c(S, 77777), s(S | A, 0, 77778), c(A, 77778, 1)]
CONVERSATIONS = [CONV_SERVER_CLOSES, CONV_CLIENT_CLOSES, CONV_BOTH_CLOSE, CONV_4WHS, CONV_KEEPALIVE, CONV_WSCALE,
                 CONV_REUSE]


def run(script, cisn=1000, sisn=5000, ssn=None, cnt=None):
    """The script through the model: [(reason, state after)], the session, the counters."""
    ssn = ssn or m.Session()
    cnt = cnt or m.Counters()
    res = [(m.step(ssn, p, cnt), ssn.state) for p in packets(script, cisn, sisn)]
    return res, ssn, cnt


ISNS = [(1000, 5000), (0xFFFFFFF0, 0xFFFFFFFF), (0x7FFFFFF0, 0x80000010), (0xFFFFFC00, 0x00000007)]


def generate(seed=20240521, per_trigger=12, per_conversation=10):
    """A mixed sequence [(flow, Pkt)]: every trigger per_trigger times and every conversation per_conversation times,
    each on a flow of its own with ISNs drawn from the seed (every fourth flow from ISNS, which wrap 2^32 or cross
    2^31), the flows' packets interleaved at random with each flow's order kept.  The seed is fixed so that every
    state is reached and every reachable reason appears at least 10 times (tests/test_stream_session_model.py)."""
    rng = np.random.default_rng(seed)
    scripts = [pre + steps for _, pre, steps in TRIGGERS for _ in range(per_trigger)]
    scripts += [pre + [c(S, 0)] for pre in SHUTDOWN_STATES for _ in range(2)]
    scripts += [conv for conv in CONVERSATIONS for _ in range(per_conversation)]
    flows = []
    for f, script in enumerate(scripts):
        ci, si = ISNS[(f // 4) % len(ISNS)] if f % 4 == 0 else (int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)))
        flows.append(packets(script, ci, si))
    order = np.repeat(np.arange(len(flows)), [len(p) for p in flows])
    rng.shuffle(order)
    pos = [0] * len(flows)
    seq = []
    for f in order.tolist():
        seq.append((f, flows[f][pos[f]]))
        pos[f] += 1
    return seq


def model_run(seq):
    """generate()'s sequence through the model: per-packet reasons, the sessions by flow, the counters."""
    ssn, cnt, reasons = {}, m.Counters(), []
    for f, p in seq:
        reasons.append(m.step(ssn.setdefault(f, m.Session()), p, cnt))
    return reasons, ssn, cnt


# ---- frames: flow f is client 10.(f >> 16).(f >> 8).(f) port 20000 + f % 40000 -> server 172.16.0.1 port 80
SERVER_IP, SERVER_PORT = 0xAC100001, 80


def endpoints(f):
    return 0x0A000000 | (f & 0xFFFFFF), 20000 + f % 40000


def frame(f, p: m.Pkt, vlan=False):
    """(the frame's first bytes up to the end of the TCP header, its wire length): Ethernet [+ one VLAN tag], IPv4
    without options, TCP with a window-scale option (NOP, WS) when p.ws is set; the payload is not materialised (the
    engine reads headers; ip_len and the wire length carry payload_len)."""
    cip, cport = endpoints(f)
    sip, dip, sport, dport = (SERVER_IP, cip, SERVER_PORT, cport) if p.toclient else (cip, SERVER_IP, cport, SERVER_PORT)
    opts = b"" if p.ws is None else bytes([1, 3, 3, p.ws])
    off = 5 + len(opts) // 4
    tcp = struct.pack(">HHIIBBHHH", sport, dport, p.seq, p.ack, off << 4, p.flags, p.win, 0, 0) + opts
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp) + p.plen, 0x1234, 0, 64, 6, 0, sip, dip)
    l2 = bytes([2, 0x11, 0x22, 0x33, 0x44, 0x55, 2, 0x66, 0x77, 0x88, 0x99, 0xAA])
    l2 += struct.pack(">HHH", 0x8100, 5, 0x0800) if vlan else struct.pack(">H", 0x0800)
    head = l2 + ip + tcp
    return head, len(head) + p.plen


def batch(seq, stride=144, vlan_every=0):
    """(hdr [n, stride] u8, len [n] u32) of a [(flow, Pkt)] sequence."""
    hdr = np.zeros((len(seq), stride), np.uint8)
    lens = np.zeros(len(seq), np.uint32)
    for i, (f, p) in enumerate(seq):
        head, wire = frame(f, p, vlan=bool(vlan_every) and f % vlan_every == 0)
        hdr[i, :len(head)] = np.frombuffer(head, np.uint8)
        lens[i] = wire
    return hdr, lens


def flow_key(f):
    cip, cport = endpoints(f)
    return (cip, SERVER_IP, cport, SERVER_PORT)
