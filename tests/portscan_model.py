"""Serial Python model of the reference's port-scan detector with an explicit clock, for the tests.

PortScan_Detect and PortScan_timeout of dataplane/src/attack/dp_portscan.c (citations are to that file unless another
is named), one packet at a time in batch index order, as one core runs them.  cvmx_get_cycle() and
OCT_TIME_SECONDS_SINCE1970 are the values of clock(); oct_cpu_rate is cycles_per_second; the record pool holds
`capacity` records (MEM_POOL_PORTSCAN_BUFFER_NUM).

The oracle assumes portscan_able = 0 (oracle/ppe_oracle.c:406).  expected() takes the oracle's classify_batch result
for a batch and rewrites exactly the packets PortScan_Detect refuses (flow.c:215-230), like tests/stream_model.py does
for StreamTcp, and then applies that model when a StreamTcp setting is given."""
import numpy as np

import stream_model as sm
from ppe import abi
from ppe.abi import ST

OK, NOMEM, DETECTED, HOLD = 0, 1, 2, 3   # dp_portscan.h:19-22
U64 = (1 << 64) - 1
U32 = (1 << 32) - 1
RESULTS = ("ok", "nomem", "detected", "hold")


class PortScanModel:
    def __init__(self, able=1, action=0, exception_freq=50, hold_seconds=600, capacity=100000,
                 cycles_per_second=10**9):
        self.able, self.action, self.freq, self.hold_seconds = able, action, exception_freq, hold_seconds  # :9-11
        self.capacity, self.rate = capacity, cycles_per_second
        self.now_cycles = self.now_seconds = 0
        self.table = {}   # sip -> pcb_t fields (dp_portscan.h:25-35)
        self.counts = dict(new_pcb=0, del_pcb=0, ok=0, nomem=0, detected=0, hold=0, drop=0)

    def clock(self, now_cycles, now_seconds):
        self.now_cycles, self.now_seconds = now_cycles & U64, now_seconds & U64

    def process(self, pcb, dport, ts):
        """PortScan_Detec_process (:139-210), verbatim."""
        now, rate = self.now_cycles, self.rate
        if pcb["hold"]:                                            # :143
            if ts < pcb["hold"]:                                   # :145
                return HOLD
            pcb["hold"] = 0                                        # :151
        if pcb["last_dport"] == 0:                                 # :155 first create
            pcb["last_dport"] = dport
            pcb["last_cycle"] = now
            return OK
        dl = (now - pcb["last_cycle"]) & U64
        if dl < rate:                                              # :163
            if pcb["last_dport"] != dport:
                pcb["last_dport"] = dport
                pcb["exception"] = (pcb["exception"] + 1) & U32
                if pcb["last_exception"] >= self.freq:             # :170
                    pcb["hold"] = (self.now_seconds + self.hold_seconds) & U64
                    return DETECTED
        elif rate < dl < ((2 * rate) & U64):                       # :177-178
            pcb["last_cycle"] = (pcb["last_cycle"] + rate) & U64
            pcb["last_exception"] = pcb["exception"]
            pcb["exception"] = 0
            if pcb["last_dport"] != dport:
                pcb["last_dport"] = dport
                pcb["exception"] = 1
                if pcb["last_exception"] >= self.freq:             # :188
                    pcb["hold"] = (self.now_seconds + self.hold_seconds) & U64
                    return DETECTED
        else:                                                      # :195 (exactly rate, >= 2 rate, wrapped)
            pcb["last_cycle"] = now
            pcb["last_exception"] = 0
            pcb["exception"] = 0
            if pcb["last_dport"] != dport:
                pcb["last_dport"] = dport
                pcb["exception"] = 1
        return OK

    def detect(self, sip, dport, ts):
        """PortScan_Detect (:231-272); None when the detector is disabled (:238-241)."""
        if self.able != 1:
            return None
        pcb = self.table.get(sip)                                  # PortScanFind :96-118
        if pcb is None:
            if len(self.table) >= self.capacity:                   # pcb_create fails :256-261
                r = NOMEM
                self.counts["nomem"] += 1
                return r
            pcb = dict(last_dport=0, exception=0, last_exception=0, last_cycle=0, cycle=0, hold=0)  # :132-134
            self.table[sip] = pcb
            self.counts["new_pcb"] += 1                            # :265
        pcb["cycle"] = self.now_cycles                             # FCB_UPDATE_TIMESTAMP :109, :263
        r = self.process(pcb, dport, ts)
        self.counts[RESULTS[r]] += 1
        return r

    def timeout(self, now_cycles):
        """PortScan_timeout (:43-93) with FRAG_MAX_TIMEOUT = 20 * oct_cpu_rate (decode-defrag.h:92)."""
        dead = [s for s, p in self.table.items() if now_cycles > p["cycle"] and now_cycles - p["cycle"] > 20 * self.rate]
        for s in dead:
            del self.table[s]
        self.counts["del_pcb"] += len(dead)
        return len(dead)

    def records(self):
        """The table as a set of (sip, last_dport, exception, last_exception, last_cycle, cycle, hold)."""
        return {(s, p["last_dport"], p["exception"], p["last_exception"], p["last_cycle"], p["cycle"], p["hold"])
                for s, p in self.table.items()}

    def info(self):
        return dict(self.counts, live=len(self.table))

    def batch(self, sip, dport, ts):
        """The detector over one batch of eligible packets; returns the result per packet."""
        return [self.detect(int(s), int(d), int(t)) for s, d, t in zip(sip, dport, ts)]

    def expected(self, ref, hdr, ts=None, now_seconds=0, stream=None):
        """ref = the oracle's classify_batch result for hdr (portscan off).  A packet reaches PortScan_Detect iff it
        reached DP_Acl_Lookup there (PPE_F_ACL; flow.c:204-232); mbuf->timestamp is ts[i] or now_seconds.  For any result
        but OK with action 0 (flow.c:216-230): status PORTSCAN_DROP, action DROP, acl_hit -1, PPE_F_ACL clear, and in
        the counters no ACL_* / FLOW_PROC_OK / OUT_FW but FLOW_PROC_FAIL (:281-282) and OUT_DROP.  Returns verdict /
        flow_hash / acl_hit / tuple / counters (array) / results (per packet, -1 = not seen) and, with `stream` (a
        stream_model setting), `stream` and `counters` as stream_model.expected returns them."""
        verdict, hit = ref["verdict"].copy(), ref["acl_hit"].copy()
        cnt = ref["counters"].astype(np.int64).copy()
        C = {k: i for i, k in enumerate(abi.COUNTERS)}
        res = np.full(len(verdict), -1, np.int64)
        if self.able == 1:
            for i in np.flatnonzero((verdict >> 16) & abi.F_ACL):
                t = int(ts[i]) if ts is not None else now_seconds
                r = self.detect(int(ref["tuple"][i][0]), int(ref["tuple"][i][2]) >> 16, t)
                res[i] = r
                if r != OK and self.action == 0:
                    self.counts["drop"] += 1                       # STAT_ATTACK_PORTSCAN_DROP flow.c:226
                    st, fl = int(verdict[i]) & 0xFF, int(verdict[i]) >> 16
                    if st == ST["ACL_FW"]:
                        for k, d in (("acl_fw", -1), ("flow_proc_ok", -1), ("out_fw", -1), ("flow_proc_fail", 1),
                                     ("out_drop", 1)):
                            cnt[C[k]] += d
                    else:
                        assert st == ST["ACL_DROP"]
                        cnt[C["acl_drop"]] -= 1
                    verdict[i] = ST["PORTSCAN_DROP"] | (abi.ACT_DROP << 8) | ((fl & ~abi.F_ACL) << 16)
                    hit[i] = -1
        out = dict(verdict=verdict, flow_hash=ref["flow_hash"], acl_hit=hit, tuple=ref["tuple"],
                   counters=cnt.astype(np.uint64), results=res)
        if stream is not None:
            e = sm.expected(out, hdr, stream)
            out.update(verdict=e["verdict"], counters=e["counters"], stream=e["stream"])
        else:
            out["counters"] = dict(zip(abi.COUNTERS, (int(x) for x in out["counters"])))
        return out
