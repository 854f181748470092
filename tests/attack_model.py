"""Serial Python model of the reference's land, SYN-flood and UDP-flood monitors with an explicit clock, for the tests.

dataplane/src/attack/dp_attack.c (citations are to that file unless another is named), one packet at a time in batch
index order, as one core runs them: the hold flags are really set by the first packet the speed branch drops and
really read by the packets after it, and the tick is DP_Attack_Info_Update verbatim.  Nothing here knows of the
engine's per-interval decision word, so a comparison with the engine tests that the verdicts do not depend on the
order of the packets between two ticks instead of assuming it.  OCT_TIME_SECONDS_SINCE1970 is the value of clock() /
tick(); attrule and attinfo are per input port (OCT_PHY_PORT_MAX = 4, oct-port.h:14); ATTACK_ENABLE is 1, so a rule
word holding 2 is off, and drop_pack == 1 means drop.

The oracle has no monitors.  expected() takes the oracle's classify_batch result for a batch and rewrites exactly the
packets a monitor drops, like tests/stream_model.py and tests/portscan_model.py do, and composes with both in the
reference's order: monitors (decode-ipv4.c:141-149, decode-tcp.c:162-173) -> syn_check -> PortScan_Detect -> ACL ->
syncount_accum (FlowAdd, flow.c:151-154) -> StreamTcp (flow.c:311)."""
import numpy as np

import stream_model as sm
from ppe import abi
from ppe.abi import ST

U64 = (1 << 64) - 1
PORTS = 4
PD_FIELDS = ("drop_pack", "land", "teardrop", "pingdeath", "pingdeath_value")          # dp_attack.h:26-33
TD_FIELDS = ("drop_pack", "flood_ping", "ping_speed", "last_ping_flood_time", "flood_udp", "udp_speed",
             "last_udp_flood_time", "flood_syn", "syn_speed", "last_syn_flood_time", "syn_count")  # :35-48
STATE = abi.ATTACK_STATE_FIELDS
TOTALS = abi.ATTACK_TOTALS
ENABLE = 1


class AttackModel:
    def __init__(self, pd=None, td=None, hold_seconds=600):
        self.ai = [dict.fromkeys(STATE, 0) for _ in range(PORTS)]      # attinfo.ai[], zeroed (:452)
        self.totals = dict.fromkeys(TOTALS, 0)                         # attstat.land / udpspeed / synspeed / syncount
        self.now = 0
        self.set(pd, td, hold_seconds)

    def set(self, pd=None, td=None, hold_seconds=600):
        """The rule file load over DP_Attack_Del_All (:33-36): {port: {field: value}}, the rest 0; flood_hold_time."""
        self.pd = [dict.fromkeys(PD_FIELDS, 0) for _ in range(PORTS)]
        self.td = [dict.fromkeys(TD_FIELDS, 0) for _ in range(PORTS)]
        for p, d in (pd or {}).items():
            self.pd[p].update(d)
        for p, d in (td or {}).items():
            self.td[p].update(d)
        self.hold_seconds = hold_seconds

    def cfg(self) -> abi.AttackCfg:
        return abi.AttackCfg.make(dict(enumerate(self.pd)), dict(enumerate(self.td)), self.hold_seconds)

    def clock(self, now_seconds):
        self.now = now_seconds & U64

    def tick(self, now_seconds):
        """DP_Attack_Info_Update (:712-748)."""
        self.clock(now_seconds)
        for a in self.ai:
            a["udppps"], a["udp_accum"] = a["udp_accum"], 0            # :724-725
            if self.now >= a["udp_flood_hold_time"]:                   # :727 (>=; also when nothing is held)
                a["udp_flood_hold"] = a["udp_flood_hold_time"] = 0
            a["synpps"], a["syn_accum"] = a["syn_accum"], 0            # :735-736
            if self.now >= a["syn_flood_hold_time"]:                   # :738
                a["syn_flood_hold"] = a["syn_flood_hold_time"] = 0
            a["syncount"], a["syncount_accum"] = a["syncount_accum"], 0  # :744-745

    def udp(self, port) -> bool:
        """DP_Attack_UdpPacketMonitor (:582-634): True = DECODE_DROP."""
        a, td = self.ai[port], self.td[port]
        a["udp_accum"] += 1                                            # :601
        if td["flood_udp"] == ENABLE:                                  # :604
            if a["udp_flood_hold"]:                                    # :606
                if td["drop_pack"] == ENABLE:
                    self.totals["udpflood_drop"] += 1
                    return True
            if a["udppps"] > td["udp_speed"]:                          # :618 uint64 > uint32, strict
                if td["drop_pack"] == ENABLE:
                    a["udp_flood_hold"] = 1                            # :626-627
                    a["udp_flood_hold_time"] = (self.now + self.hold_seconds) & U64
                    self.totals["udpflood_drop"] += 1
                    return True
        return False

    def syn(self, port, sip, dip):
        """decode-tcp.c:162-173: DP_Land_Attack_Monitor (:464-484), then DP_Attack_SynPacketMonitor (:637-688).
        Returns the engine status of the drop, or None."""
        pd, a, td = self.pd[port], self.ai[port], self.td[port]
        if pd["land"] == ENABLE and dip == sip and pd["drop_pack"] == ENABLE:
            self.totals["land_drop"] += 1
            return ST["ATTACK_LAND"]                                   # (not counted in syn_accum: it returned)
        a["syn_accum"] += 1                                            # :641
        if td["flood_syn"] == ENABLE:                                  # :643
            if a["syn_flood_hold"]:
                if td["drop_pack"] == ENABLE:
                    self.totals["synflood_drop"] += 1
                    return ST["ATTACK_SYNFLOOD"]
            if a["synpps"] > td["syn_speed"]:                          # :657
                if td["drop_pack"] == ENABLE:
                    a["syn_flood_hold"] = 1                            # :665-666
                    a["syn_flood_hold_time"] = (self.now + self.hold_seconds) & U64
                    self.totals["synflood_drop"] += 1
                    return ST["ATTACK_SYNFLOOD"]
        if a["syncount"] > td["syn_count"]:                            # :673 (not gated by flood_syn)
            if td["drop_pack"] == ENABLE:
                self.totals["syncount_drop"] += 1
                return ST["ATTACK_SYNCOUNT"]
        return None

    def info(self) -> dict:
        return dict(ai=[dict(a) for a in self.ai], **self.totals)

    def expected(self, ref, hdr, ports=None, portscan=None, ts=None, now_seconds=0, stream=None):
        """ref = the oracle's classify_batch result for hdr; ports = the packets' input-port bytes (None: port 0; the
        engine takes port & 3); portscan = a PortScanModel or None; stream = a stream_model setting or None.

        Who reaches a monitor, from the oracle's result: the UDP monitor every packet DecodeIPV4 hands to DecodeUDP
        (status UDP_HEADER_ERR / UDP_LEN_ERR, or a UDP packet that reached the flow engine), the SYN monitors every TCP
        packet that reached the flow engine (it passed DecodeTCP's three length checks) with SYN.  WINDOW_PUNT and
        fragments reach none.  A monitor drop: action DROP, acl_hit -1, flow hash 0, flags VLAN as decoded plus
        TCP | SYN on the SYN monitors' statuses, tuple {sip, dip, 0, proto | vlan << 8}; in the counters what the
        reference has counted by then (up to IPV4_RX_OK) and OUT_DROP."""
        verdict, hit = ref["verdict"].copy(), ref["acl_hit"].copy()
        fh, tup = ref["flow_hash"].copy(), ref["tuple"].copy()
        cnt = dict(zip(abi.COUNTERS, (int(x) for x in ref["counters"])))
        n = len(verdict)
        port_of = (lambda i: 0) if ports is None else (lambda i: int(ports[i]) & 3)
        undo = {  # what the packet had counted past IPV4_RX_OK in the oracle's run
            ("u", ST["UDP_HEADER_ERR"]): ("udp_headerlen_err",), ("u", ST["UDP_LEN_ERR"]): ("udp_pktlen_err",),
            ("u", ST["ACL_FW"]): ("udp_rx_ok", "acl_fw", "flow_proc_ok", "out_fw"),
            ("u", ST["ACL_DROP"]): ("udp_rx_ok", "acl_drop", "flow_proc_fail"),
            ("t", ST["ACL_FW"]): ("tcp_rx_ok", "acl_fw", "flow_proc_ok", "out_fw"),
            ("t", ST["ACL_DROP"]): ("tcp_rx_ok", "acl_drop", "flow_proc_fail")}
        for i in range(n):
            v = int(verdict[i])
            st, fl = v & 0xFF, v >> 16
            l4, tcp = bool(fl & abi.F_L4), bool(fl & abi.F_TCP)
            new = None
            if st in (ST["UDP_HEADER_ERR"], ST["UDP_LEN_ERR"]) or (l4 and not tcp):
                kind = "u"
                if self.udp(port_of(i)):
                    new = ST["ATTACK_UDPFLOOD"]
            elif l4 and tcp and (fl & abi.F_SYN):
                kind = "t"
                new = self.syn(port_of(i), int(tup[i][0]), int(tup[i][1]))
            if new is None:
                continue
            for k in undo[(kind, st)]:
                cnt[k] -= 1
            if st == ST["ACL_FW"]:
                cnt["out_drop"] += 1
            nf = (fl & abi.F_VLAN) | ((abi.F_TCP | abi.F_SYN) if kind == "t" else 0)
            verdict[i] = new | (abi.ACT_DROP << 8) | (nf << 16)
            hit[i] = -1
            fh[i] = 0
            tup[i][2] = 0
            tup[i][3] = int(tup[i][3]) & 0x1FF
        out = dict(verdict=verdict, flow_hash=fh, acl_hit=hit, tuple=tup,
                   counters=np.array([cnt[k] for k in abi.COUNTERS], np.uint64))
        if portscan is not None:  # a monitor drop lost PPE_F_ACL above: it never reaches PortScan_Detect
            e = portscan.expected(out, hdr, ts=ts, now_seconds=now_seconds)
            out.update(verdict=e["verdict"], acl_hit=e["acl_hit"],
                       counters=np.array([e["counters"][k] for k in abi.COUNTERS], np.uint64))
        # DP_Attack_SynCountMonitor in FlowAdd (flow.c:151-154): every TCP SYN the ACL forwarded, before StreamTcp
        need = abi.F_TCP | abi.F_SYN
        for i in np.flatnonzero(((out["verdict"] & 0xFF) == ST["ACL_FW"]) & (((out["verdict"] >> 16) & need) == need)):
            self.ai[port_of(i)]["syncount_accum"] += 1
        e = sm.expected(out, hdr, stream if stream is not None else sm.OFF)
        out.update(verdict=e["verdict"], counters=e["counters"], stream=e["stream"])
        return out


# ---- frames for the known answers (tests/pktbuild.py): one of each class the monitors tell apart ----
KINDS = ("udp", "udp_short", "udp_lenerr", "syn", "synack", "ack", "syn_lenerr", "syn_hdrerr", "frag", "icmp", "rst")


def frame(kind, sip=0x0A000001, dip=0x0A000002, vlan_tag=False, ihl=5, dport=80) -> bytes:
    """udp: good; udp_short: l4len 4 < 8 (UDP_HEADER_ERR); udp_lenerr: uh_len != l4len; syn / synack / ack / rst: good
    TCP with those flags; syn_lenerr: SYN with data offset 4 (TCP_LEN_ERR); syn_hdrerr: SYN flags in a 16-byte TCP
    header (TCP_HEADER_ERR); frag: a UDP first fragment; icmp: protocol 1."""
    from pktbuild import eth, ipv4, tcp, udp, vlan
    l2 = (eth(0x8100) + vlan(0x0800)) if vlan_tag else eth(0x0800)
    tf = dict(syn=0x02, synack=0x12, ack=0x10, rst=0x04, syn_lenerr=0x02, syn_hdrerr=0x02)
    if kind == "udp":
        l4, proto = udp(1234, dport, b"\0" * 18), 17
    elif kind == "udp_short":
        l4, proto = b"\x04\xd2\x00\x50", 17
    elif kind == "udp_lenerr":
        l4, proto = udp(1234, dport, b"\0" * 18, ulen=99), 17
    elif kind == "frag":
        l4, proto = udp(1234, dport, b"\0" * 16), 17
    elif kind == "icmp":
        l4, proto = b"\x08\x00" + b"\0" * 14, 1
    elif kind == "syn_hdrerr":
        l4, proto = tcp(1234, dport, 0x02)[:16], 6
    else:
        l4, proto = tcp(1234, dport, tf[kind], off=4 if kind == "syn_lenerr" else 5, payload=b"\0" * 6), 6
    off = 0x2000 if kind == "frag" else 0
    return l2 + ipv4(proto, sip, dip, len(l4), ihl=ihl, off=off) + l4


def batch(frames, stride=64):
    """(hdr (n, stride) u8, len (n,) u32) of a list of frames: the first `stride` bytes each, zero-padded."""
    hdr = np.zeros((len(frames), stride), np.uint8)
    for i, f in enumerate(frames):
        b = np.frombuffer(f[:stride], np.uint8)
        hdr[i, :len(b)] = b
    return hdr, np.array([len(f) for f in frames], np.uint32)
