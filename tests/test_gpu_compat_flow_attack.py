"""The land, SYN-flood, SYN-count and UDP-flood monitors ahead of the flow table behind Decode (include/ppe_decode.h:
flow_attack_able, DP_Attack_*): a connection, a land SYN and a UDP flood through Decode at bursts of 1, 64 and 300 with
input_port 0..3 and DP_Attack_Tick between the bursts, against the serial model (tests/attack_flow_model.py); how a
status 25-28 mbuf is delivered; the switch 0 -> 1 -> 0; the detector as well (the shim's ppe_flow_combine); the rule
load and DP_Attack_Del_All; the release; four threads.  Integer work: no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import portscan_model as psm  # noqa: E402
from attack_flow_model import AttackFlowModel  # noqa: E402
from attack_model import AttackModel  # noqa: E402
from flow_combined_model import FlowCombinedModel  # noqa: E402
from pktbuild import tcp_packet, udp_packet  # noqa: E402
from ppe import Attack, abi  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_compat_flow import DIR, Session, check_delivery, frames_to_windows, got, setg, web_rules  # noqa: E402
from test_gpu_flow import table  # noqa: E402

RATE = 10**9
NOW = 1_700_000_000
CL, SRV, SCAN = 0x0A000001, 0x0A000002, 0x0A000063
HOLD = 50
KNOBS = dict(flow_attack_able=0, flow_portscan_able=0, flood_hold_time=600, portscan_exception_freq=50, portscan_action=0)
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
# port 0: land and a UDP flood above 4 packets a second; port 1: a SYN flood above 2; port 2: the count monitor above 1
# created flow a second; port 3: every monitor on with drop_pack 2 (nothing drops)
PD = {0: dict(drop_pack=1, land=1), 3: dict(drop_pack=2, land=1)}
TD = {0: dict(drop_pack=1, flood_udp=1, udp_speed=4, syn_count=1 << 30),
      1: dict(drop_pack=1, flood_syn=1, syn_speed=2, syn_count=1 << 30),
      2: dict(drop_pack=1, syn_count=1),
      3: dict(drop_pack=2, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=0)}


class AtkSession(Session):
    def __init__(self, rules, pd=PD, td=TD, detector=False, **kw):
        super().__init__(rules, **kw)
        lib = self.lib
        atk = AttackModel(None, None, HOLD)
        if detector:
            fp = fpm.FlowPortScanModel(self.oracle, 100000, psm.PortScanModel(1, 0, 2, HOLD, 100000, RATE))
            self.m = FlowCombinedModel(self.oracle, atk, fp)
        else:
            self.m = AttackFlowModel(self.oracle, 100000, atk)
        self.detector = detector
        setg(lib, flow_able=1, flow_attack_able=1, flood_hold_time=HOLD, flow_portscan_able=1 if detector else 0,
             portscan_exception_freq=2)
        self.rules_set(pd, td)
        self.clock(NOW, 10 * RATE)

    def rules_set(self, pd, td):
        self.m.atk.set(pd, td, HOLD)
        cfg = self.m.atk.cfg()
        cfg.hold_seconds = 7                      # (ignored: the shim's hold time is flood_hold_time)
        assert self.lib.DP_Attack_Rule_Set(C.byref(cfg)) == 0

    def clock(self, now, cycles=None):
        self.lib.DP_Attack_Clock(now)
        self.lib.DP_Flow_Clock(now)
        self.m.atk.clock(now)
        if cycles is not None:
            self.lib.DP_PortScan_Clock(cycles, now)
            if self.detector:
                self.m.fp.ps.clock(cycles, now)
        self.now = now

    def tick(self, now):
        assert self.lib.DP_Attack_Tick(now) == 0
        self.m.atk.tick(now)
        self.lib.DP_Flow_Clock(now)
        self.now = now

    def obj(self):
        """The shim's monitor object as an Attack (for info); not owned."""
        a = Attack.__new__(Attack)
        a.eng, a.lib, a.h = self.engine(), self.lib, C.c_void_p(self.lib.DP_Attack_Object())
        assert a.h
        return a

    def run(self, frames, burst, ports):
        hdr, lens = frames_to_windows(frames)
        n = len(lens)
        ports = np.asarray(ports, np.uint8)
        self.lib.Decode_Set_Burst(burst)
        self.load(hdr, lens)
        for i in range(n):
            self.mbufs[i].timestamp = self.now
            self.mbufs[i].input_port = int(ports[i])
        self.decode(0, n)
        assert self.lib.Decode_Flush() == n % burst
        cfg = self.oracle.cfg(0, 1, self.now)
        ts = np.full(n, self.now, np.uint64)
        parts = []
        for lo in range(0, n, burst):
            sl = slice(lo, lo + burst)
            parts.append(self.m.classify_batch(hdr[sl], lens[sl], ports[sl], ts[sl], cfg) if self.detector else
                         self.m.classify_batch(hdr[sl], lens[sl], ports[sl], cfg=cfg))
        ref = {k: np.concatenate([p[k] for p in parts]) for k in ("verdict", "acl_hit")}
        check_delivery(self, ref, n)              # (statuses 25-28 are not among the logged ones: no DP_Log_Func)
        return ref

    def same(self):
        info, want = self.obj().info(), self.m.info()
        for p in range(4):
            g = {k: info["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
            assert g == want["ai"][p], ("port", p, g, want["ai"][p])
        assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}
        assert info["cfg"]["hold_seconds"] == HOLD
        mt = self.m.table() if self.detector else table(self.m.ft.dump())
        assert table(self.engine().flow_dump()) == mt

    def close(self):
        setg(self.lib, **KNOBS)
        self.lib.DP_Attack_Clock(0)
        self.lib.DP_PortScan_Clock(0, 0)
        super().close()


def traffic(r):
    """Round r, with each frame's input port: a connection to port 80 on port 1, a land SYN on port 0 and one on port 3,
    six UDP packets of one flow on port 0, three SYNs of new flows on port 2, three SYNs of one flow on port 1."""
    conn = [tcp_packet(CL, SRV, 40000 + r, 80, flags=0x02), tcp_packet(SRV, CL, 80, 40000 + r, flags=0x12),
            tcp_packet(CL, SRV, 40000 + r, 80, flags=0x10)]
    land = [tcp_packet(SRV, SRV, 50000 + r, 80, flags=0x02)] * 2
    udp = [udp_packet(CL, SRV, 6000, 80)] * 6
    new = [tcp_packet(CL + 16 + k, SRV, 41000 + r, 80, flags=0x02) for k in range(3)]
    rep = [tcp_packet(CL + 32, SRV, 42000, 80, flags=0x02)] * 3
    return conn + land + udp + new + rep, [1, 1, 1, 0, 3] + [0] * 6 + [2] * 3 + [1] * 3


@pytest.mark.parametrize("burst", [1, 64, 300])
def test_connection_land_and_flood_through_decode(burst):
    """Second 0: only the land SYN on port 0 drops (no rate is known yet).  Second 1: the UDP flood (udppps 6 > 4) and
    the SYN flood (synpps 5 > 2) arm their holds, port 2's count monitor (syncount 3 > 1) drops every SYN; port 3 counts
    and drops nothing.  The counts land per port."""
    s = AtkSession(web_rules())
    try:
        fr, ports = traffic(0)
        r0 = s.run(fr, burst, ports)
        st = (r0["verdict"] & 0xFF).tolist()
        assert st[3] == LAND and st[4] == ST["ACL_FW"] and st.count(LAND) == 1
        assert not set(st) & {SYNF, SYNC, UDPF}
        ai = s.obj().info()["ai"]
        assert [ai[p]["udp_accum"] for p in range(4)] == [6, 0, 0, 0]
        assert [ai[p]["syn_accum"] for p in range(4)] == [0, 5, 3, 1]          # SYN and SYN|ACK of the connection, 3 repeats
        assert [ai[p]["syncount_accum"] for p in range(4)] == [0, 2, 3, 1]     # the flows SYNs created, by port
        s.same()
        s.tick(NOW + 1)
        fr1, p1 = traffic(1)
        r1 = s.run(fr1 + fr * 20, burst, p1 + ports * 20)                     # (several bursts of 64, more than one of 300)
        st = r1["verdict"] & 0xFF
        assert (st == UDPF).sum() == 6 * 21 and (st == SYNC).sum() == 3 * 21 and (st == LAND).sum() == 21
        assert (st == SYNF).sum() == 5 * 21                                   # (a SYN|ACK counts as a SYN; three repeats)
        info = s.obj().info()
        assert info["ai"][0]["udp_flood_hold_time"] == NOW + 1 + HOLD and info["ai"][1]["syn_flood_hold"] == 1
        assert (info["land_drop"], info["udpflood_drop"], info["syncount_drop"]) == (22, 126, 63)
        s.same()
        s.tick(NOW + 2)
        s.tick(NOW + 3)                                                       # every rate 0; the holds stay
        r2 = s.run(fr, burst, ports)
        st = (r2["verdict"] & 0xFF).tolist()
        assert st.count(UDPF) == 6 and st.count(SYNC) == 0 and st.count(SYNF) == 5
        s.same()
    finally:
        s.close()


def test_status_25_to_28_delivery_and_mbuf_fields():
    """The drop hook, no DP_Log_Func, no PKT_HAS_FLOW, no direction flag, ports 0; the UDP-flood monitor sits ahead of
    DecodeUDP (no transport header), the TCP monitors behind DecodeTCP's length checks."""
    s = AtkSession(web_rules())
    try:
        fr, ports = traffic(0)
        s.run(fr, 64, ports)
        s.tick(NOW + 1)
        ref = s.run(fr, 64, ports)
        st = ref["verdict"] & 0xFF
        assert {LAND, SYNF, SYNC, UDPF} <= set(st.tolist())
        act = dict(s.seen)
        v, hit, fl = got(s, len(st))
        for i in np.flatnonzero(np.isin(st, (LAND, SYNF, SYNC, UDPF))):
            m = s.mbufs[int(i)]
            assert act[int(i)] == abi.ACT_DROP and int(i) not in s.logged
            assert fl[i] & DIR == 0 and hit[i] == -1 and (m.sport, m.dport) == (0, 0)
            assert m.network_header and m.sip in (CL, SRV, CL + 32) + tuple(CL + 16 + k for k in range(3))
            assert bool(m.transport_header) == (st[i] != UDPF) and m.proto == (17 if st[i] == UDPF else 6)
        assert not s.logged
    finally:
        s.close()


def test_switch_off_on_off():
    """flow_attack_able 0 -> 1 -> 0: with it off the verdicts are those of a session that never set it; the object keeps
    its rules and counts while detached; without flow_able the global has no effect."""
    def session(switch):
        s = AtkSession(web_rules())
        out = []
        try:
            fr, ports = traffic(0)
            for r in range(3):
                on = switch and r == 1
                setg(s.lib, flow_attack_able=1 if on else 0)
                s.lib.Decode_Set_Burst(64)
                hdr, lens = frames_to_windows(fr)
                s.load(hdr, lens)
                for i in range(len(lens)):
                    s.mbufs[i].input_port = ports[i]
                s.decode(0, len(lens))
                assert s.lib.Decode_Flush() == len(lens)
                v, hit, fl = got(s, len(lens))
                out.append((v.tobytes(), hit.tobytes(), (fl & DIR).tobytes(), list(s.seen)))
                if r >= 1 and switch:
                    ai = s.obj().info()["ai"]
                    assert [ai[p]["udp_accum"] for p in range(4)] == [6, 0, 0, 0]      # counted once, kept while detached
                    assert s.obj().info()["cfg"]["pd"][0]["land"] == 1
            setg(s.lib, flow_able=0, flow_attack_able=1)       # the stateless path: no monitors, no refusal
            hdr, lens = frames_to_windows(fr)
            s.load(hdr, lens)
            s.decode(0, len(lens))
            assert s.lib.Decode_Flush() == len(lens)
            out.append(got(s, len(lens))[0].tobytes())
            return out, table(s.engine().flow_dump())
        finally:
            s.close()
    (a, _), (b, _) = session(False), session(True)
    assert a[0] == b[0] and a[3] == b[3]                       # before it was set, and the stateless path
    # round 1: no rate is known yet, so the one difference is the land SYN on port 0 (its flow exists since round 0)
    va, vb = np.frombuffer(a[1][0], np.uint32), np.frombuffer(b[1][0], np.uint32)
    assert np.flatnonzero(va != vb).tolist() == [3] and vb[3] & 0xFF == LAND and va[3] & 0xFF == ST["ACL_FW"]
    assert dict(b[1][3])[3] == abi.ACT_DROP and dict(a[1][3])[3] == abi.ACT_FW
    assert a[2] == b[2]                                        # off again: every verdict, flag and hook as without it


def test_detector_as_well_runs_the_combined_path():
    """flow_portscan_able = 1 too: the shim turns ppe_flow_combine on for its context; a scanner's status 24 and a land
    drop in one burst, one launch of kind 3."""
    s = AtkSession(web_rules(), detector=True)
    try:
        scan = lambda r: [tcp_packet(SCAN, SRV, 50000 + r, p, flags=0x02) for p in (21, 22, 23, 80, 25, 443, 8080)]  # noqa: E731
        land = [tcp_packet(SRV, SRV, 50000, 80, flags=0x02)]
        r0 = s.run(scan(0) + land, 64, [1] * 7 + [0])
        assert (r0["verdict"] & 0xFF).tolist()[-1] == LAND and ST["PORTSCAN_DROP"] not in (r0["verdict"] & 0xFF).tolist()
        assert s.engine().flow_launch_info() == (3, 1)
        s.clock(NOW + 1, 11 * RATE + RATE // 2)                              # the detector's window rolls
        r1 = s.run(scan(1) + land + scan(1), 64, [1] * 7 + [0] + [1] * 7)
        st = (r1["verdict"] & 0xFF).tolist()
        assert st.count(ST["PORTSCAN_DROP"]) >= 7 and st[7] == LAND
        assert s.engine().flow_launch_info() == (3, 1)
        act = dict(s.seen)
        mine = [i for i, x in enumerate(st) if x in (LAND, ST["PORTSCAN_DROP"])]
        assert all(act[i] == abi.ACT_DROP for i in mine) and not set(mine) & set(s.logged)
        s.same()
        ps = s.m.fp.ps.info()
        assert ps["drop"] >= 7
        # the switch stays on for the context with only the monitors attached: nothing changes (kind 4 for a small burst)
        setg(s.lib, flow_portscan_able=0)
        s.m.fp.ps.able = 0
        s.run(land + scan(2)[:2], 64, [0, 1, 1])
        assert s.engine().flow_launch_info() == (4, 1)
    finally:
        s.close()


def test_rule_set_del_all_and_hold_time():
    s = AtkSession(web_rules())
    try:
        fr, ports = traffic(0)
        s.run(fr, 64, ports)
        s.tick(NOW + 1)
        assert s.obj().info()["cfg"]["hold_seconds"] == HOLD                  # not the argument's 7
        s.lib.DP_Attack_Del_All()
        s.m.atk.set(None, None, HOLD)
        r = s.run(fr, 64, ports)
        assert not set((r["verdict"] & 0xFF).tolist()) & {LAND, SYNF, SYNC, UDPF}
        info = s.obj().info()
        assert info["cfg"]["pd"][0]["land"] == 0 and info["ai"][0]["udp_accum"] == 6 and info["land_drop"] == 1
        s.same()
        setg(s.lib, flood_hold_time=9)                                        # read per flush
        s.m.atk.set(PD, TD, 9)
        cfg = s.m.atk.cfg()
        assert s.lib.DP_Attack_Rule_Set(C.byref(cfg)) == 0
        s.tick(NOW + 2)
        r = s.run(fr, 1, ports)
        assert (r["verdict"] & 0xFF == UDPF).sum() == 6
        info = s.obj().info()
        assert info["cfg"]["hold_seconds"] == 9 and info["ai"][0]["udp_flood_hold_time"] == NOW + 2 + 9
        setg(s.lib, flood_hold_time=HOLD)
        s.m.atk.set(PD, TD, HOLD)
        s.run(fr[:3], 1, ports[:3])                                           # the flush alone takes the new hold time
        assert s.obj().info()["cfg"]["hold_seconds"] == HOLD
    finally:
        s.close()


def test_release_then_a_fresh_start():
    s = AtkSession(web_rules())
    try:
        fr, ports = traffic(0)
        s.run(fr, 64, ports)
        assert s.lib.DP_Attack_Object()
        s.lib.DP_Acl_Rule_Release()                                           # the object goes before its context
        assert not s.lib.DP_Attack_Object() and not s.lib.ppe_compat_ctx()
        assert s.lib.DP_Attack_Tick(NOW + 1) == 0
        s.commit()
        s.m.close()
        s.m = AttackFlowModel(s.oracle, 100000, AttackModel(None, None, HOLD))
        s.m.atk.clock(NOW + 1)                                                # (DP_Attack_Tick's clock is kept)
        r = s.run(fr, 64, ports)                                              # all-zero rules again, fresh counts
        assert not set((r["verdict"] & 0xFF).tolist()) & {LAND, SYNF, SYNC, UDPF}
        s.same()
    finally:
        s.close()


def test_four_threads():
    """Four threads, each its own input port and its own flows, at burst 1 with all-zero rules: the counts land per port
    whatever the order across threads, and every mbuf has its thread's own verdict."""
    per, T = 10, 4
    fr = []
    for t in range(T):
        c = 0x0A010000 + (t << 8)
        for k in range(per):
            fr += [tcp_packet(c, SRV, 30000 + k, 80, flags=0x02), tcp_packet(SRV, c, 80, 30000 + k, flags=0x12),
                   udp_packet(c, SRV, 30000 + k, 80), tcp_packet(c, SRV, 30000 + k, 80, flags=0x10)]
    hdr, lens = frames_to_windows(fr)
    n, each = len(lens), 4 * per
    s = AtkSession(web_rules(), pd=None, td=None)
    try:
        s.lib.Decode_Set_Burst(1)
        s.load(hdr, lens)
        for i in range(n):
            s.mbufs[i].timestamp = NOW
            s.mbufs[i].input_port = i // each
        th = [threading.Thread(target=s.decode, args=(each * t, each * (t + 1))) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join(60)
        assert not any(x.is_alive() for x in th)
        ports = (np.arange(n) // each).astype(np.uint8)
        parts = [s.m.classify_batch(hdr[i:i + 1], lens[i:i + 1], ports[i:i + 1], cfg=s.oracle.cfg(0, 1, NOW))
                 for i in range(n)]
        ref = {k: np.concatenate([p[k] for p in parts]) for k in ("verdict", "acl_hit")}
        check_delivery(s, ref, n)
        ai = s.obj().info()["ai"]
        assert [(ai[p]["udp_accum"], ai[p]["syn_accum"], ai[p]["syncount_accum"]) for p in range(4)] == [(per, 2 * per, per)] * 4
        s.same()
    finally:
        s.close()
