"""The attack monitors ahead of the flow table, as the reference runs them: Decode -> DecodeIPV4 / DecodeTCP (monitors,
decode-ipv4.c:141-149, decode-tcp.c:162-173) -> FlowHandlePacket -> FlowFind | syn_check -> ACL -> FlowAdd
(flow.c:181-245), for the tests of ppe_flow_attack_attach.

Nothing new is modelled here: tests/attack_model.py's AttackModel.udp() / .syn() (dp_attack.c:582-634, :464-484,
:637-688, cited there line by line) judge each packet serially in batch index order, so the hold flags are really set
and read in order and nothing assumes the verdicts' order independence; pyoracle.OracleFlow (the oracle's sequential
FlowHandlePacket, pinned to flow.c by tests/test_oracle_flow.py) then sees only the packets no monitor dropped, in their
order.  A dropped packet's row is written as AttackModel.expected writes it.  The one difference from the stateless
composition (AttackModel.expected): DP_Attack_SynCountMonitor is called from FlowAdd behind flow_item_alloc
(flow.c:120-158, the call at :151-154 under TCP_IS_SYN), so syncount_accum counts the TCP SYN packets that create their
flow (PPE_F_NEWFLOW), not every forwarded SYN."""
import numpy as np

import pyoracle
from attack_model import AttackModel
from ppe import abi
from ppe.abi import ST


class AttackFlowModel:
    def __init__(self, oracle: pyoracle.Oracle, capacity: int, atk: AttackModel):
        self.o = oracle
        self.ft = pyoracle.OracleFlow(oracle, capacity=capacity)
        self.atk = atk

    def close(self):
        self.ft.close()

    def judge(self, hdr, lens, ports, cfg, punt=None):
        """Per packet, in index order: the status of the monitor drop or None.  Who reaches which monitor is read from
        the stateless oracle's decode result by the rule of AttackModel.expected's docstring: the UDP monitor every
        packet DecodeIPV4 hands to DecodeUDP (UDP_HEADER_ERR / UDP_LEN_ERR, or a UDP packet that reached the flow
        engine), the land / SYN monitors every TCP packet that reached the flow engine with SYN; WINDOW_PUNT and
        fragments reach none (punt: the packets the engine punts at its window, whatever the oracle reads behind it).
        Whether the packet's flow exists plays no part: the monitors sit ahead of FlowFind."""
        dec = self.o.classify_batch(hdr, lens, cfg=cfg)
        port_of = (lambda i: 0) if ports is None else (lambda i: int(ports[i]) & 3)
        drops = [None] * len(lens)
        for i in range(len(lens)):
            v = int(dec["verdict"][i])
            st, fl = v & 0xFF, v >> 16
            l4, tcp = bool(fl & abi.F_L4), bool(fl & abi.F_TCP)
            if punt is not None and punt[i]:
                continue
            if st in (ST["UDP_HEADER_ERR"], ST["UDP_LEN_ERR"]) or (l4 and not tcp):
                if self.atk.udp(port_of(i)):
                    drops[i] = ST["ATTACK_UDPFLOOD"]
            elif l4 and tcp and (fl & abi.F_SYN):
                drops[i] = self.atk.syn(port_of(i), int(dec["tuple"][i][0]), int(dec["tuple"][i][1]))
        return dec, drops

    def classify_batch(self, hdr, lens, ports=None, cfg=None, punt=None):
        """One batch: verdict, flow_hash, acl_hit, tuple, counters (np.uint64[32], abi.COUNTERS order) and `dropped`
        (the monitor-dropped indices); the flow table, the monitors' state and totals move as the reference's would.
        punt (bool per packet, or None): the frames whose decode needs a byte past the engine's window
        (tests/decode_corpus.py expected(): reach > stride).  The engine punts them ahead of every monitor and of the
        flow table; their rows and counters are written as decode_corpus.expected writes them."""
        hdr = np.ascontiguousarray(hdr, np.uint8)
        lens = np.ascontiguousarray(lens, np.uint32)
        cfg = cfg or self.o.cfg()
        n = len(lens)
        dec, drops = self.judge(hdr, lens, ports, cfg, punt)
        away = np.zeros(n, bool) if punt is None else np.asarray(punt, bool)
        keep = np.array([i for i in range(n) if drops[i] is None and not away[i]], np.int64)
        gone = np.array([i for i in range(n) if drops[i] is not None], np.int64)
        out = dict(verdict=np.zeros(n, np.uint32), flow_hash=np.zeros(n, np.uint32), acl_hit=np.full(n, -1, np.int32),
                   tuple=np.zeros((n, 4), np.uint32), counters=np.zeros(32, np.uint64), dropped=gone)
        if len(keep):  # the survivors, in order, through FlowHandlePacket
            ref = self.ft.classify_batch(hdr[keep], lens[keep], cfg=cfg)
            for k in ("verdict", "flow_hash", "acl_hit", "tuple"):
                out[k][keep] = ref[k]
            out["counters"] += ref["counters"]
            # DP_Attack_SynCountMonitor in FlowAdd (flow.c:151-154): the TCP SYN packets that created their flow
            need = abi.F_NEWFLOW | abi.F_TCP | abi.F_SYN
            for j in np.flatnonzero(((ref["verdict"] >> 16) & need) == need):
                i = int(keep[j])
                self.atk.ai[0 if ports is None else int(ports[i]) & 3]["syncount_accum"] += 1
        cnt = dict(zip(abi.COUNTERS, (int(x) for x in out["counters"])))
        for i in gone:  # as AttackModel.expected writes a monitor drop
            fl = int(dec["verdict"][i]) >> 16
            tcp_syn = drops[i] != ST["ATTACK_UDPFLOOD"]
            nf = (fl & abi.F_VLAN) | ((abi.F_TCP | abi.F_SYN) if tcp_syn else 0)
            out["verdict"][i] = drops[i] | (abi.ACT_DROP << 8) | (nf << 16)
            out["tuple"][i] = dec["tuple"][i]
            out["tuple"][i][2] = 0
            out["tuple"][i][3] = int(dec["tuple"][i][3]) & 0x1FF
            # what the reference has counted by then: the RX chain up to IPV4_RX_OK (and the received bytes), then
            # output_drop_proc
            for k in ("pkts", "l2_rx_ok", "ipv4_rx_ok", "out_drop") + (("vlan_rx_ok",) if fl & abi.F_VLAN else ()):
                cnt[k] += 1
            cnt["rx_bytes"] += int(lens[i])
        for i in np.flatnonzero(away):  # WINDOW_PUNT: PUNT, the VLAN flag, addresses and protocol only
            fl = int(dec["verdict"][i]) >> 16
            out["verdict"][i] = ST["WINDOW_PUNT"] | (abi.ACT_PUNT << 8) | ((fl & abi.F_VLAN) << 16)
            out["tuple"][i] = (dec["tuple"][i][0], dec["tuple"][i][1], 0, int(dec["tuple"][i][3]) & 0xFF)
            for k in ("pkts", "window_punt", "out_punt", "l2_rx_ok", "ipv4_rx_ok") + \
                    (("vlan_rx_ok",) if fl & abi.F_VLAN else ()):
                cnt[k] += 1
            cnt["rx_bytes"] += int(lens[i])
        out["counters"] = np.array([cnt[k] for k in abi.COUNTERS], np.uint64)
        return out

    def age(self, now, timeout=20):
        return self.ft.age(now, timeout)

    def info(self):
        return self.atk.info()
