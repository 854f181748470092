"""The port-scan detector on the flow table's misses behind Decode (include/ppe_decode.h: flow_portscan_able): a
connection and a scanner through Decode at bursts of 1, 64 and 300 with both clocks moved between the bursts, against the
serial model (tests/flow_portscan_model.py); how a status-24 mbuf is delivered; the switch 0 -> 1 -> 0; DP_PortScan_Age;
four threads over disjoint flows and sources.  Integer work: no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import portscan_model as psm  # noqa: E402
from pktbuild import tcp_packet, udp_packet  # noqa: E402
from ppe import PortScan, abi  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_compat_flow import DIR, Session, check_delivery, frames_to_windows, got, setg, web_rules  # noqa: E402
from test_gpu_flow import table  # noqa: E402

RATE = 10**9  # Decode's detector: 1e9 cycles are one second
CL, SRV, SCAN = 0x0A000001, 0x0A000002, 0x0A000063
FREQ, HOLD = 2, 50
KNOBS = dict(portscan_action=0, portscan_exception_freq=50, flood_hold_time=600, flow_portscan_able=0)


class PsSession(Session):
    def __init__(self, rules, **kw):
        super().__init__(rules, **kw)
        self.lib.DP_PortScan_Table.restype = C.c_void_p
        self.m = fpm.FlowPortScanModel(self.oracle, 100000, psm.PortScanModel(1, 0, FREQ, HOLD, 100000, RATE))
        setg(self.lib, flow_able=1, flow_portscan_able=1, portscan_exception_freq=FREQ, flood_hold_time=HOLD)

    def clock(self, cycles, seconds):
        self.lib.DP_PortScan_Clock(cycles, seconds)
        self.lib.DP_Flow_Clock(seconds)
        self.m.ps.clock(cycles, seconds)
        self.now = seconds

    def table_obj(self):
        """The shim's port-scan table as a PortScan (for info / dump); not owned."""
        p = PortScan.__new__(PortScan)
        p.eng, p.lib, p.h = self.engine(), self.lib, C.c_void_p(self.lib.DP_PortScan_Table())
        assert p.h
        return p

    def run(self, frames, burst, ts=None):
        """The frames through Decode in bursts, and through the model (burst by burst, as the flushes take them)."""
        hdr, lens = frames_to_windows(frames)
        n = len(lens)
        self.lib.Decode_Set_Burst(burst)
        self.load(hdr, lens)
        for i in range(n):
            self.mbufs[i].timestamp = int(ts[i]) if ts is not None else self.now
        self.decode(0, n)
        assert self.lib.Decode_Flush() == n % burst
        tsa = np.array([self.mbufs[i].timestamp for i in range(n)], np.uint64)
        parts = [self.m.classify_batch(hdr[lo:lo + burst], lens[lo:lo + burst], tsa[lo:lo + burst],
                                       self.oracle.cfg(0, 1, self.now)) for lo in range(0, n, burst)]
        ref = {k: np.concatenate([p[k] for p in parts]) for k in ("verdict", "acl_hit", "results")}
        check_delivery(self, ref, n)
        return ref

    def same(self):
        e, p = self.engine(), self.table_obj()
        assert table(e.flow_dump()) == self.m.table()
        assert fpm.ps_records(p.dump()) == self.m.ps.records()
        pi, mi = p.info(), self.m.ps.info()
        assert all(pi[k] == mi[k] for k in ("live", "new_pcb", "del_pcb", "ok", "nomem", "detected", "hold", "drop"))

    def close(self):
        setg(self.lib, **KNOBS)
        self.lib.DP_PortScan_Clock(0, 0)
        super().close()


def traffic(r):
    """Round r: a connection to port 80 (SYN, SYN|ACK, ACK) and a scanner's SYNs to eight ports of the same server, port
    80 among them, then the connection's ACK again."""
    conn = [tcp_packet(CL, SRV, 40000 + r, 80, flags=0x02), tcp_packet(SRV, CL, 80, 40000 + r, flags=0x12),
            tcp_packet(CL, SRV, 40000 + r, 80, flags=0x10)]
    scan = [tcp_packet(SCAN, SRV, 50000 + r, p, flags=0x02) for p in (21, 22, 23, 80, 25, 443, 8080, 80)]
    return conn + scan + [tcp_packet(SCAN, SRV, 50000 + r, 80, flags=0x10)] + conn[2:]


@pytest.mark.parametrize("burst", [1, 64, 300])
def test_connection_and_scanner_through_decode(burst):
    """Round 0 (quiet): the scanner's port changes only count, its SYN to port 80 creates a flow.  Round 1, 1.5 s later:
    the window rolls, the first change is DETECTED and the rest HOLD (status 24), while the scanner's own flow of round
    0 and the client's connection pass.  Round 2, after the hold: the scanner is judged afresh."""
    s = PsSession(web_rules())
    try:
        s.clock(10 * RATE, 1000)
        r0 = s.run(traffic(0), burst)
        assert (r0["results"] == psm.OK).sum() == 8 and not (r0["verdict"] & 0xFF == ST["PORTSCAN_DROP"]).any()
        s.clock(11 * RATE + RATE // 2, 1001)
        r1 = s.run(traffic(1) + traffic(0) * 28, burst)   # (several bursts of 64, more than one of 300)
        st = r1["verdict"] & 0xFF
        assert (r1["results"] == psm.DETECTED).sum() == 1 and (r1["results"] == psm.HOLD).sum() == 7 + 28 * 6
        assert (st == ST["PORTSCAN_DROP"]).sum() == (r1["results"] > 0).sum() and (st == ST["ACL_FW"]).sum() > 100
        s.same()
        s.clock(14 * RATE, 1001 + HOLD)
        r2 = s.run(traffic(2), burst)
        assert not (r2["results"] == psm.HOLD).any() and (r2["results"] == psm.OK).sum() == 8
        s.same()
    finally:
        s.close()


def test_status_24_delivery_and_mbuf_fields():
    s = PsSession(web_rules())
    try:
        s.clock(10 * RATE, 1000)
        s.run(traffic(0), 64)
        s.clock(11 * RATE + RATE // 2, 1001)
        ref = s.run(traffic(1), 64)
        dropped = np.flatnonzero(ref["verdict"] & 0xFF == ST["PORTSCAN_DROP"])
        assert len(dropped) >= 7
        act = dict(s.seen)
        v, hit, fl = got(s, len(ref["verdict"]))
        for i in dropped:
            m = s.mbufs[int(i)]
            assert act[int(i)] == abi.ACT_DROP and int(i) not in s.logged          # the drop hook, no DP_Log_Func
            assert fl[i] & DIR == 0 and hit[i] == -1                               # no PKT_HAS_FLOW, no direction
            assert (m.sport, m.sip, m.proto) == (50001, SCAN, 6) and m.dport in (21, 22, 23, 80, 25, 443, 8080)
    finally:
        s.close()


def test_switch_off_on_off():
    """flow_portscan_able 0 -> 1 -> 0: the runs with it off are byte-identical to a session that never set it; the table
    keeps its records while detached; without flow_able the global has no effect."""
    def session(switch):
        s = PsSession(web_rules())
        out = []
        try:
            setg(s.lib, flow_portscan_able=0)
            s.m.ps.able = 0
            for r in range(3):
                on = switch and r == 1
                setg(s.lib, flow_portscan_able=1 if on else 0)
                s.m.ps.able = 1 if on else 0
                s.clock((10 + 2 * r) * RATE, 1000 + r)
                ref = s.run(traffic(0) + traffic(r), 64)
                v, hit, fl = got(s, len(ref["verdict"]))
                out.append((v.tobytes(), hit.tobytes(), (fl & DIR).tobytes(), list(s.seen)))
                if switch and r >= 1:
                    p = s.table_obj()
                    assert p.info()["live"] == 2 and fpm.ps_records(p.dump()) == s.m.ps.records()
                else:
                    assert not s.lib.DP_PortScan_Table()
            setg(s.lib, flow_able=0, flow_portscan_able=1)   # the stateless path: no detector, no refusal
            s.lib.Decode_Set_Burst(64)
            hdr, lens = frames_to_windows(traffic(5))
            s.load(hdr, lens)
            s.decode(0, len(lens))
            assert s.lib.Decode_Flush() == len(lens)
            out.append(got(s, len(lens))[0].tobytes())
            return out, table(s.engine().flow_dump())
        finally:
            s.close()
    (a, ta), (b, tb) = session(False), session(True)
    assert a[0] == b[0] and a[3] == b[3]          # before it was set, and the stateless path
    # round 2 runs with it off again on a table round 1 left differently (the detector dropped nothing there: quiet
    # windows), so every round and the table agree
    assert a == b and ta == tb


def test_portscan_age_behind_decode():
    s = PsSession(web_rules())
    try:
        s.clock(10 * RATE, 1000)
        s.run(traffic(0), 64)
        freed = C.c_uint64(9)
        assert s.lib.DP_PortScan_Age(10 * RATE + 20 * RATE, C.byref(freed)) == 0 and freed.value == 0   # not yet (:70)
        assert s.lib.DP_PortScan_Age(10 * RATE + 20 * RATE + 1, C.byref(freed)) == 0 and freed.value == 2
        assert s.m.ps.timeout(10 * RATE + 20 * RATE + 1) == 2
        s.same()
        s.clock(40 * RATE, 1030)
        s.run(traffic(1), 64)
        s.same()
    finally:
        s.close()


def test_four_threads_disjoint_flows_and_sources():
    """Four threads each Decode their own clients' connections and port probes at burst 1: the flows and the sources are
    disjoint, so the order across threads does not matter: every mbuf has the verdict of its thread's own sequence."""
    per, T = 12, 4
    fr = []
    for t in range(T):
        c = 0x0A010000 + (t << 8)
        for k in range(per):
            fr += [tcp_packet(c, SRV, 30000 + k, 80, flags=0x02), tcp_packet(SRV, c, 80, 30000 + k, flags=0x12),
                   udp_packet(c, SRV, 30000 + k, 1000 + k), tcp_packet(c, SRV, 30000 + k, 80, flags=0x10)]
    hdr, lens = frames_to_windows(fr)
    n, each = len(lens), 4 * per
    s = PsSession(web_rules())
    try:
        s.clock(10 * RATE, 1000)
        s.lib.Decode_Set_Burst(1)
        s.load(hdr, lens)
        for i in range(n):
            s.mbufs[i].timestamp = 1000
        th = [threading.Thread(target=s.decode, args=(each * t, each * (t + 1))) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join(60)
        assert not any(x.is_alive() for x in th)
        parts = [s.m.classify_batch(hdr[i:i + 1], lens[i:i + 1], np.array([1000], np.uint64), s.oracle.cfg(0, 1, 1000))
                 for i in range(n)]
        ref = {k: np.concatenate([p[k] for p in parts]) for k in ("verdict", "acl_hit", "results")}
        check_delivery(s, ref, n)
        # the server's replies are found (never at the detector); each client's probes change its port per connection
        assert (ref["results"] == psm.OK).sum() == 2 * T * per and s.table_obj().info()["live"] == T
        s.same()
    finally:
        s.close()
