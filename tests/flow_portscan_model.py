"""Serial Python model of the reference's FlowGetFlowFromHash with PortScan_Detect inside, for the tests of
ppe_flow_portscan_attach.

One packet at a time in batch index order, as one core runs dataplane/src/flow/flow.c (citations are to that file unless
another is named):
    FlowFind (:96-118, :196-201)      found: STAT_ACL_FW, no ACL lookup, never at the detector
    syn_check (:204-214)              a TCP miss without SYN: FLOW_TCP_NO_SYN_FIRST, the detector is not called
    PortScan_Detect (:215-230)        any result but OK with portscan_action 0: STAT_ATTACK_PORTSCAN_DROP, return NULL
    DP_Acl_Lookup (:232-243)          DROP: STAT_ACL_DROP, no flow; else STAT_ACL_FW
    FlowAdd (:120-158)                flow_item_alloc fails: STAT_FLOW_NODE_NOMEM (:124-129); else the flow, oriented as
                                      this packet
    FlowHandlePacket (:271-310)       direction (:248-269), FlowUpdate (:163-178), PKT_HAS_FLOW, STAT_FLOW_PROC_OK; NULL
                                      above: output_drop_proc, STAT_FLOW_PROC_FAIL (:281-282)
Decode, the flow hash, the tuple, syn_check and the ACL's verdict of every packet are read from the stateless oracle's
row for it (pyoracle.Oracle.classify_batch: every packet a miss, no detector); the detector is
tests/portscan_model.py's PortScanModel.detect; the flow table is the small Python one below, pinned to
pyoracle.OracleFlow by tests/test_flow_portscan_model.py (able = 0 over the same batches).  The counters start from the
stateless oracle's and move, per packet whose row differs from its stateless row, by the STAT_ lines that differ."""
from collections import Counter

import numpy as np

import portscan_model as psm
from ppe import abi
from ppe.abi import ST

C = {k: i for i, k in enumerate(abi.COUNTERS)}
FLOWBITS = abi.F_FLOW | abi.F_TOCLIENT | abi.F_NEWFLOW


def flow_key(sip, dip, sport, dport, proto):
    """FlowMatch (:81-94): the 5-tuple in either direction."""
    a, b = (sip, sport), (dip, dport)
    return (proto,) + (a + b if a <= b else b + a)


class FlowPortScanModel:
    def __init__(self, oracle, capacity, ps: psm.PortScanModel):
        self.o, self.capacity, self.ps = oracle, capacity, ps
        self.flows = {}        # flow_key -> flow_item_t fields (flow.h:55-72)
        self.new_flow = self.del_flow = 0
        self.events = Counter()  # what the generated batches must contain (tests/test_flow_portscan_model.py)

    # ---- one packet ----
    def _forward(self, f, sip, sport, dport, wire_len, now):
        """FlowGetPacketDirection (:248-269), FlowUpdate (:163-178), FLOW_UPDATE_TIMESTAMP: the direction flag."""
        to_server = (f["sport"] == sport) if sport != dport else (f["sip"] == sip)
        if sport == f["sport"]:
            f["pktcnts2d"] += 1
            f["bytecnts2d"] += wire_len
        else:
            f["pktcntd2s"] += 1
            f["bytecntd2s"] += wire_len
        f["last_seen"] = now
        return abi.F_FLOW | (0 if to_server else abi.F_TOCLIENT)

    def classify_batch(self, hdr, lens, ts=None, cfg=None):
        """One batch: verdict, flow_hash, acl_hit, tuple, counters (np.uint64[32], abi.COUNTERS order), results (per
        packet PortScan_Detect's answer, -1 = not called)."""
        hdr = np.ascontiguousarray(hdr, np.uint8)
        lens = np.ascontiguousarray(lens, np.uint32)
        cfg = cfg or self.o.cfg()
        now = int(cfg.now_seconds)
        dec = self.o.classify_batch(hdr, lens, cfg=cfg)
        n = len(lens)
        verdict, hit = dec["verdict"].copy(), dec["acl_hit"].copy()
        cnt = dec["counters"].astype(np.int64).copy()
        res = np.full(n, -1, np.int64)
        claimers, creator = {}, {}  # per tuple missing as the batch starts: its would-be creators; its creator

        def move(i, st, flags, hitv, deltas):
            verdict[i] = st | ((abi.ACT_FW if st == ST["ACL_FW"] else abi.ACT_DROP) << 8) | (flags << 16)
            hit[i] = hitv
            for k, d in deltas:
                cnt[C[k]] += d

        for i in range(n):
            v = int(dec["verdict"][i])
            st0, fl = v & 0xFF, v >> 16
            if not fl & abi.F_L4:          # never reached FlowHandlePacket
                continue
            sip, dip, w2, w3 = (int(x) for x in dec["tuple"][i])
            sport, dport, proto = w2 & 0xFFFF, w2 >> 16, w3 & 0xFF
            key = flow_key(sip, dip, sport, dport, proto)
            wl = int(lens[i])
            # what the stateless row counted behind the RX chain, to be taken back when the row changes
            undo = {ST["ACL_FW"]: [("acl_fw", -1), ("flow_proc_ok", -1), ("out_fw", -1)],
                    ST["ACL_DROP"]: [("acl_drop", -1), ("flow_proc_fail", -1), ("out_drop", -1)],
                    ST["FLOW_TCP_NO_SYN_FIRST"]: [("flow_tcp_no_syn_first", -1), ("flow_proc_fail", -1),
                                                  ("out_drop", -1)]}[st0]
            if st0 == ST["ACL_FW"] and key not in self.flows:
                claimers.setdefault(key, []).append(i)
            f = self.flows.get(key)
            if f is not None:              # :196-201 found; FlowHandlePacket :284-309
                pcb = self.ps.table.get(sip)
                t = int(ts[i]) if ts is not None else now
                if self.ps.able == 1 and pcb is not None and pcb["hold"] and t < pcb["hold"]:
                    self.events["found_of_held_source"] += 1
                bits = self._forward(f, sip, sport, dport, wl, now)
                move(i, ST["ACL_FW"], (fl & ~(abi.F_ACL | FLOWBITS)) | bits, -1,
                     undo + [("acl_fw", 1), ("flow_proc_ok", 1), ("out_fw", 1)])
                continue
            if st0 == ST["FLOW_TCP_NO_SYN_FIRST"]:   # :204-214
                continue
            t = int(ts[i]) if ts is not None else now
            r = self.ps.detect(sip, dport, t)        # :215
            if r is not None:
                res[i] = r
                self.events[psm.RESULTS[r]] += 1
                if r != psm.OK and self.ps.action == 0:   # :216-230
                    self.ps.counts["drop"] += 1
                    move(i, ST["PORTSCAN_DROP"], fl & ~abi.F_ACL, -1, undo + [("flow_proc_fail", 1), ("out_drop", 1)])
                    continue
            if st0 == ST["ACL_DROP"]:                # :232-237
                continue
            if len(self.flows) >= self.capacity:     # FlowAdd :124-129 (STAT_ACL_FW stays counted, :240)
                if r == psm.OK:
                    self.events["nomem_after_ok"] += 1
                move(i, ST["FLOW_NOMEM"], fl, int(dec["acl_hit"][i]),
                     [("flow_proc_ok", -1), ("out_fw", -1), ("flow_node_nomem", 1), ("flow_proc_fail", 1),
                      ("out_drop", 1)])
                continue
            f = dict(sip=sip, dip=dip, sport=sport, dport=dport, protocol=proto, pktcnts2d=0, pktcntd2s=0,
                     bytecnts2d=0, bytecntd2s=0, last_seen=now)
            self.flows[key] = f
            self.new_flow += 1
            creator[key] = i
            bits = self._forward(f, sip, sport, dport, wl, now)
            move(i, ST["ACL_FW"], fl | bits | abi.F_NEWFLOW, int(dec["acl_hit"][i]), [])
        for key, idx in claimers.items():
            if key not in creator:
                self.events["creatorless_claim"] += 1
            elif creator[key] != idx[0]:
                self.events["creator_not_lowest"] += 1
        return dict(verdict=verdict, flow_hash=dec["flow_hash"], acl_hit=hit, tuple=dec["tuple"],
                    counters=cnt.astype(np.uint64), results=res)

    # ---- the tables ----
    def age(self, now, timeout=20):
        """FlowAgeTimeoutCB (:391-467): now > last_seen && now - last_seen > timeout."""
        dead = [k for k, f in self.flows.items() if now > f["last_seen"] and now - f["last_seen"] > timeout]
        for k in dead:
            del self.flows[k]
        self.del_flow += len(dead)
        return len(dead)

    def table(self):
        """The flows as tests/test_gpu_flow.py's table() lists a dump."""
        cols = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s",
                "last_seen")
        return sorted(tuple(f[c] for c in cols) for f in self.flows.values())

    def stats(self):
        return dict(live=len(self.flows), new_flow=self.new_flow, del_flow=self.del_flow)


def ps_records(dump):
    """A ppe_portscan_dump / PortScan.dump() array as PortScanModel.records() lists the table."""
    return {tuple(int(dump[c][k]) for c in ("sip", "last_dport", "exception", "last_exception", "last_cycle", "cycle",
                                            "hold")) for k in range(len(dump))}


# ---- the generated batches of the GPU tests ----
SRC = [0x0A000000 + 16 * k + 1 for k in range(8)]     # 8 sources
SRV = [0x0B000001, 0x0B000002]                        # two servers
PORTS = [80, 81, 82, 443, 8080, 9]                    # 6 ports: 9 has no rule (ACL DROP)
RATE = 1000                                           # cycles per second of the generator's detector


def gen_rules():
    """FW to ports 80, 81, 82, 443 and 8080 and from them (the replies); everything else is the default DROP."""
    r = np.zeros(10, abi.RULE_DTYPE)
    for k, p in enumerate(PORTS[:5]):
        r[k]["sport_end"] = 65535
        r[k]["dport_start"] = r[k]["dport_end"] = p
        r[k + 5]["dport_end"] = 65535
        r[k + 5]["sport_start"] = r[k + 5]["sport_end"] = p
    r["protocol_end"] = 255
    r["action"] = abi.ACL_RULE_ACTION_FW
    return r


def gen_batch(rng, n, stride=64):
    """n packets of 8 sources towards 6 ports of two servers, both directions, TCP (SYN, SYN|ACK, ACK) and UDP, few client
    ports so that tuples repeat inside and across batches; per packet a timestamp around the batch's second."""
    from pktbuild import tcp_packet, udp_packet
    hdr = np.zeros((n, stride), np.uint8)
    lens = np.zeros(n, np.uint32)
    for i in range(n):
        c, s = SRC[int(rng.integers(8))], SRV[int(rng.integers(2))]
        cp, sp = 40000 + int(rng.integers(4)), PORTS[int(rng.integers(6))]
        rev = rng.random() < 0.3
        if rng.random() < 0.6:
            fl = 0x12 if rev and rng.random() < 0.7 else 0x02 if rng.random() < 0.6 else 0x10
            f = tcp_packet(s, c, sp, cp, flags=fl) if rev else tcp_packet(c, s, cp, sp, flags=fl)
        else:
            f = udp_packet(s, c, sp, cp) if rev else udp_packet(c, s, cp, sp)
        hdr[i, :len(f)] = np.frombuffer(f, np.uint8)
        lens[i] = len(f)
    return hdr, lens


def gen_sequence(seed, batches, max_n, freq=2, flow_capacity=None, ps_capacity=8, hold=2):
    """The schedule of the generated test: per batch (hdr, lens, ts, now_seconds, now_cycles, age) with the clock stepped
    so that all three time branches of PortScan_Detec_process occur (< rate, between rate and 2 rate, beyond, and now and
    then far enough for PortScan_timeout), holds expire inside batches, and both tables are aged now and then."""
    rng = np.random.default_rng(seed)
    if flow_capacity is None:  # (a pool that a few batches fill and the aging empties again)
        flow_capacity = max(64, max_n // 3)
    now_s, now_c = 1000, 10 * RATE
    out = []
    for b in range(batches):
        n = int(rng.integers(1, max_n + 1)) if b % 5 else int(rng.choice([1, 63, 64, 65, max_n - 1, max_n]))
        hdr, lens = gen_batch(rng, n)
        step = int(rng.choice([0, RATE // 3, RATE + RATE // 2, 3 * RATE, 25 * RATE], p=[0.3, 0.3, 0.3, 0.06, 0.04]))
        now_c += step
        now_s += int(rng.integers(0, 3))
        ts = (now_s + rng.integers(0, 3, n)).astype(np.uint64)
        out.append(dict(hdr=hdr, lens=lens, ts=ts, now_s=now_s, now_c=now_c, age=(b % 4 == 3)))
    return out, dict(freq=freq, flow_capacity=flow_capacity, ps_capacity=ps_capacity, hold=hold, rate=RATE)
