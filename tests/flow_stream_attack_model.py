"""The attack monitors, the flow table and the TCP sessions on one batch (ppe_flow_stream_monitors), as the reference
runs them: Decode -> DecodeIPV4 / DecodeTCP (monitors) -> FlowHandlePacket (FlowAdd: DP_Attack_SynCountMonitor,
flow.c:151-154; flow_item_t.input_port, flow.c:139) -> StreamTcp (flow.c:304-320).

A composition, nothing re-modelled: tests/attack_flow_model.py's AttackFlowModel judges every packet with the serial
monitors, runs the survivors through the oracle's flow table and counts syncount_accum's +1;
tests/stream_session_model.py's step() then takes every TCP packet that has a flow, in index order, exactly as
tests/test_gpu_flow_stream.py's Rig does.  What this file adds is the reference's three decrements:

  DP_Attack_SynCountFins (stream-tcp.c:608 in the 4WHS branch :582-617, :660 in the 3WHS branch), each directly behind
  StreamTcpPacketSetState(ssn, TCP_ESTABLISHED) (:609, :661), on the completing packet's m->input_port: a step that
  takes the session from SYN_RECV to ESTABLISHED.  With midstream and async_oneside 0 the other three sites of that
  state change (:382, :698, :956) are dead, so the rule is the state before and after the step
  (tests/golden/ref_stream_syncount_v1.npz holds the reference's own calls, packet by packet);

  StreamTcp_Flow_ResRelease (stream-tcp-session.c:61-77, from FlowAgeResRelease, flow.c:413-419): a flow that ages out
  with protoctx != NULL and state <= TCP_SYN_RECV, on the flow's input_port.  The engine's ssn == NULL is state NONE.

The arithmetic is cvmx_atomic_add64 on a uint64_t: modulo 2^64."""
import numpy as np

import stream_session_model as m
from attack_flow_model import AttackFlowModel
from attack_model import U64
from ppe import abi

OUT_FW, OUT_DROP = abi.COUNTERS.index("out_fw"), abi.COUNTERS.index("out_drop")
NEED = abi.F_FLOW | abi.F_TCP


def ends(sip, dip, sport, dport):
    """A flow's key whatever the direction: the two (address, port) ends, sorted."""
    return tuple(sorted(((int(sip), int(sport)), (int(dip), int(dport)))))


class FlowStreamAttackModel:
    def __init__(self, oracle, capacity, atk):
        self.afm = AttackFlowModel(oracle, capacity, atk)
        self.o, self.ft, self.atk = oracle, self.afm.ft, atk
        self.ssn, self.port, self.cnt = {}, {}, m.Counters()

    def close(self):
        self.afm.close()

    def add(self, port, k):
        a = self.atk.ai[port]
        a["syncount_accum"] = (a["syncount_accum"] + k) & U64

    def classify_batch(self, hdr, lens, ports=None, cfg=None):
        """One batch: AttackFlowModel's result with the sessions' verdicts, and the reasons per packet."""
        out = self.afm.classify_batch(hdr, lens, ports, cfg=cfg)
        for a in self.atk.ai:  # (AttackFlowModel adds plain integers)
            a["syncount_accum"] &= U64
        v, cn = out["verdict"].copy(), out["counters"].astype(np.int64)
        reasons = np.zeros(len(lens), np.uint32)
        for i in np.flatnonzero(((v & 0xFF) == 0) & (((v >> 16) & NEED) == NEED)):
            fl, t = int(v[i]) >> 16, out["tuple"][i]
            pb = 0 if ports is None else int(ports[i]) & 3
            key = ends(t[0], t[1], int(t[2]) & 0xFFFF, int(t[2]) >> 16)
            if fl & abi.F_NEWFLOW or key not in self.ssn:
                self.ssn[key] = m.Session()
            if fl & abi.F_NEWFLOW:
                self.port[key] = pb  # flow.c:139
            row = hdr[i]
            th = 14 + (4 if (int(t[3]) >> 8) & 1 else 0)
            th += 4 * (int(row[th]) & 15)
            wso = (int(t[3]) >> 9) & 63
            p = m.Pkt(bool(fl & abi.F_TOCLIENT), int(row[th + 13]), int.from_bytes(row[th + 4:th + 8].tobytes(), "big"),
                      int.from_bytes(row[th + 8:th + 12].tobytes(), "big"),
                      int.from_bytes(row[th + 14:th + 16].tobytes(), "big"), int(t[3]) >> 16,
                      int(row[th + wso + 2]) if wso else None)
            ssn = self.ssn[key]
            before = ssn.state
            r = m.step(ssn, p, self.cnt)
            if before == m.TCP_SYN_RECV and ssn.state == m.TCP_ESTABLISHED:
                self.add(pb, -1)  # stream-tcp.c:608, :660
            if r:
                st = m.status_of(r)
                v[i] = st | (abi.ACT_DROP << 8) | ((fl | (r << abi.F_STREAM_REASON_SHIFT if st == 29 else 0)) << 16)
                cn[OUT_FW] -= 1
                cn[OUT_DROP] += 1
                reasons[i] = r
        return dict(out, verdict=v, counters=cn.astype(np.uint64)), reasons

    def tcp_keys(self):
        d = self.ft.dump()
        return {ends(e["sip"], e["dip"], e["sport"], e["dport"]) for e in d[d["protocol"] == 6]}

    def age(self, now, timeout=20, release=True):
        """FlowAgeTimeoutCB, with StreamTcp_Flow_ResRelease for every TCP flow that disappears (release False: the
        engine's aging without the decrement pass)."""
        before = self.tcp_keys()
        n = self.ft.age(now, timeout)
        for key in before - self.tcp_keys():
            ssn = self.ssn.pop(key, None)
            port = self.port.pop(key, 0)
            if release and ssn is not None and m.TCP_NONE < ssn.state <= m.TCP_SYN_RECV:
                self.add(port, -1)  # stream-tcp-session.c:70
        return n

    def sessions(self):
        """{key: (state, flags, client..., server..., port)} of every live TCP flow."""
        return {k: self.ssn.get(k, m.Session()).astuple() + (self.port.get(k, 0),) for k in self.tcp_keys()}

    def info(self):
        return self.atk.info()
