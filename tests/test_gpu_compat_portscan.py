"""The port-scan detector behind Decode (include/ppe_decode.h: portscan_able, portscan_action, portscan_exception_freq,
flood_hold_time, DP_PortScan_Clock / _Age / _Table) on the GPU: a scanner among quiet sources through Decode at burst 1,
64 and 300 against the oracle rewritten by the tests' serial model (tests/portscan_model.py), burst by burst.  Integer
work: no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loads the HIP runtime first)

import pyoracle  # noqa: E402
import test_gpu_portscan as gp  # noqa: E402  (frames, port_rules)
from portscan_model import DETECTED, HOLD, PortScanModel  # noqa: E402
from ppe import abi  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_compat import ALERT, HOOK, LOGGED, Mbuf, unhook  # noqa: E402

RATE = 10**9
N = 400
PKT_TO_SERVER, PKT_HAS_FLOW = 1 << 4, 1 << 8
GLOBALS = dict(portscan_able=0, portscan_action=0, portscan_exception_freq=50, flood_hold_time=600)


def setg(lib, **kw):
    for k, v in kw.items():
        C.c_uint32.in_dll(lib, k).value = v


class Session:
    """The compat layer with gp.port_rules() committed (default action DROP, as the library starts) and hooks that
    record (mbuf index, hook); leaves the library as it found it."""

    def __init__(self, n):
        self.lib = lib = abi.load()
        lib.ppe_set_output_hooks.argtypes = [HOOK, HOOK, HOOK]
        lib.reg_fw_alert.argtypes = [ALERT]
        assert lib.DP_Acl_Rule_Init() == 0
        lib.ppe_rule_list_free()
        assert lib.ppe_rule_list_init() == 0
        self.rules = gp.port_rules()
        for i in range(len(self.rules)):
            rid = C.c_uint32()
            assert lib.Rule_add(self.rules[i:i + 1].ctypes.data, C.byref(rid)) == 0
        assert lib.DP_Acl_Rule_Commit() == 0
        self.oracle = pyoracle.Oracle(self.rules, default_action=1)
        self.mbufs = (Mbuf * n)()
        self.base = C.addressof(self.mbufs)
        self.seen, self.logged = [], []
        idx = lambda p: (p - self.base) // C.sizeof(Mbuf)  # noqa: E731
        self.hooks = [HOOK(lambda m, a=a: self.seen.append((idx(C.addressof(m.contents)), a))) for a in (0, 1, 2)]
        self.alert = ALERT(lambda p: self.logged.append(idx(p)) or 0)
        lib.ppe_set_output_hooks(*self.hooks)
        lib.reg_fw_alert(self.alert)

    def load(self, hdr, lens, ts):
        self.bufs = [C.create_string_buffer(bytes(hdr[i]), 144) for i in range(len(lens))]
        C.memset(self.mbufs, 0, C.sizeof(self.mbufs))
        for i in range(len(lens)):
            self.mbufs[i].pkt_ptr = C.cast(self.bufs[i], C.c_void_p)
            self.mbufs[i].pkt_totallen = int(lens[i])
            self.mbufs[i].timestamp = int(ts[i])
        del self.seen[:], self.logged[:]

    def table(self):
        h = self.lib.DP_PortScan_Table()
        assert h
        info, n = abi.PortScanInfo(), C.c_uint32(0)
        assert self.lib.ppe_portscan_info(h, C.byref(info)) == 0
        assert self.lib.ppe_portscan_dump(h, None, 0, C.byref(n)) == 0
        ent = np.zeros(n.value, abi.PORTSCAN_ENTRY_DTYPE)
        if n.value:
            assert self.lib.ppe_portscan_dump(h, ent.ctypes.data, n.value, C.byref(n)) == 0
        return info.as_dict(), {tuple(int(x) for x in e) for e in ent}

    def close(self):
        setg(self.lib, **GLOBALS)
        self.lib.Decode_Set_Burst(1)
        unhook(self.lib)
        self.lib.ppe_rule_list_free()
        self.lib.DP_Acl_Rule_Release()


def scenario():
    """400 UDP frames: a scanner (a new port per packet, 1,000 .. 1,199: the FW rule) on the even indices, five quiet
    sources on the odd ones (their ports hit the FW rule, the DROP rule and the default DROP).  Timestamps: packets 300
    to 349 lie past every hold the scenario can arm, the last fifty before it again."""
    i = np.arange(N)
    sip = np.where(i % 2 == 0, gp.S0 + 1, gp.S0 + 10 + i % 5).astype(np.uint32)
    dport = np.where(i % 2 == 0, 1000 + i // 2, np.array([1500, 2500, 80, 1501, 2501])[i % 5]).astype(np.uint32)
    hdr, lens = gp.frames(sip, dport)
    ts = np.where(i < 300, 100 + i // 100, np.where(i < 350, 5000, 103)).astype(np.uint64)
    return hdr, lens, ts


def clock_at(lo):
    """The clock of the burst that starts at packet lo: the window rolls once, for the bursts from packet 100 on (at
    burst 300: for the second burst), then moves inside the window; the seconds move along."""
    k = lo // 100
    return 5 * RATE + min(k, 1) * (RATE + 1) + max(k - 1, 0) * 1000, 100 + k


def run(s, burst, model, hdr, lens, ts):
    """The scenario through Decode in bursts; returns the model's expected outputs (concatenated) when a model runs."""
    lib, n = s.lib, len(lens)
    lib.Decode_Set_Burst(burst)
    exps = []
    for lo in range(0, n, burst):
        hi = min(lo + burst, n)
        lib.DP_PortScan_Clock(*clock_at(lo))
        for i in range(lo, hi):
            lib.Decode(C.byref(s.mbufs[i]))
        if hi - lo < burst:
            assert lib.Decode_Flush() == hi - lo
        assert len(s.seen) == hi, "a burst is delivered when its last Decode (or the flush) returns"
        if model is not None:
            model.clock(*clock_at(lo))
            ref = s.oracle.classify_batch(hdr[lo:hi], lens[lo:hi], ts=ts[lo:hi], cfg=s.oracle.cfg(0, 1, 0))
            exps.append(model.expected(ref, hdr[lo:hi], ts=ts[lo:hi]))
    if not exps:
        return None
    return {k: np.concatenate([e[k] for e in exps]) for k in ("verdict", "acl_hit", "flow_hash", "results")}


def check_delivery(s, exp, n):
    assert sorted(i for i, _ in s.seen) == list(range(n)), "every mbuf reaches exactly one hook"
    v = np.array([s.mbufs[i].ppe_verdict for i in range(n)], np.uint32)
    assert np.array_equal(v, exp["verdict"]), np.flatnonzero(v != exp["verdict"])[:8]
    assert np.array_equal(np.array([s.mbufs[i].ppe_acl_hit for i in range(n)], np.int32), exp["acl_hit"])
    act = dict(s.seen)
    assert [act[i] for i in range(n)] == ((exp["verdict"] >> 8) & 0xFF).tolist()
    st = exp["verdict"] & 0xFF
    assert sorted(s.logged) == np.flatnonzero(np.isin(st, list(LOGGED))).tolist()   # status 24 is not among them
    for i in range(n):
        m = s.mbufs[i]
        flow = m.flags & (PKT_HAS_FLOW | PKT_TO_SERVER)
        if st[i] == ST["PORTSCAN_DROP"]:
            assert act[i] == 1 and i not in s.logged and flow == 0
            # the UDP decoder's fields (decode-udp.c:38-45) are there
            b, at = s.bufs[i].raw, C.addressof(s.bufs[i])
            assert (m.sport, m.dport) == ((b[34] << 8) | b[35], (b[36] << 8) | b[37]) and m.proto == 17
            assert m.transport_header == at + 34 and m.payload == at + 42 and m.sip == int.from_bytes(b[26:30], "big")
        elif st[i] == ST["ACL_FW"]:
            assert flow == PKT_HAS_FLOW | PKT_TO_SERVER


@pytest.mark.parametrize("burst", [1, 64, 300])
def test_scanner_through_decode(burst):
    hdr, lens, ts = scenario()
    s = Session(N)
    try:
        setg(s.lib, portscan_able=1, portscan_exception_freq=3, flood_hold_time=5)
        model = PortScanModel(exception_freq=3, hold_seconds=5)
        s.load(hdr, lens, ts)
        assert not s.lib.DP_PortScan_Table()                       # NULL before the first enabled flush
        exp = run(s, burst, model, hdr, lens, ts)
        check_delivery(s, exp, N)
        res = exp["results"]
        assert (res == DETECTED).any() and (res == HOLD).sum() >= 25 and (res[300:350] != HOLD).all()
        info, recs = s.table()
        assert {k: info[k] for k in gp.INFO_KEYS} == {k: model.info()[k] for k in gp.INFO_KEYS}
        assert recs == model.records() and info["cfg"]["capacity"] == 100000 and info["cfg"]["exception_freq"] == 3
        # PortScan_timeout: nothing is old enough at the last clock; everything 20 rate and a cycle later
        freed = C.c_uint64(9)
        last = clock_at((N - 1) // burst * burst)[0]
        assert s.lib.DP_PortScan_Age(last + 20 * RATE, C.byref(freed)) == 0
        assert freed.value == model.timeout(last + 20 * RATE)
        assert s.lib.DP_PortScan_Age(last + 20 * RATE + 1, C.byref(freed)) == 0
        assert freed.value == model.timeout(last + 20 * RATE + 1) > 0
        info, recs = s.table()
        assert recs == model.records() and info["live"] == model.info()["live"]
    finally:
        s.close()


def test_action_forward():
    """portscan_action = 1: detection and state run, nothing is dropped for it."""
    hdr, lens, ts = scenario()
    s = Session(N)
    try:
        setg(s.lib, portscan_able=1, portscan_action=1, portscan_exception_freq=3, flood_hold_time=5)
        model = PortScanModel(action=1, exception_freq=3, hold_seconds=5)
        s.load(hdr, lens, ts)
        exp = run(s, 64, model, hdr, lens, ts)
        check_delivery(s, exp, N)
        assert (exp["results"] == DETECTED).any() and not ((exp["verdict"] & 0xFF) == ST["PORTSCAN_DROP"]).any()
        info, recs = s.table()
        assert info["drop"] == 0 and info["detected"] == model.info()["detected"] > 0 and recs == model.records()
    finally:
        s.close()


def snapshot(s, n):
    return [C.string_at(C.addressof(s.mbufs[i]), C.sizeof(Mbuf)) for i in range(n)], list(s.seen), list(s.logged)


def test_disabled_is_identical():
    """portscan_able = 0: the mbufs (every byte) and the hook calls are those of a library that never had the detector
    on; enabling it and disabling it again leaves the same."""
    hdr, lens, ts = scenario()
    s = Session(N)
    try:
        s.load(hdr, lens, ts)                                      # (the same packet buffers in every pass)
        bufs = s.bufs

        def one_pass():
            C.memset(s.mbufs, 0, C.sizeof(s.mbufs))
            for i in range(N):
                s.mbufs[i].pkt_ptr = C.cast(bufs[i], C.c_void_p)
                s.mbufs[i].pkt_totallen = int(lens[i])
                s.mbufs[i].timestamp = int(ts[i])
            del s.seen[:], s.logged[:]
            run(s, 64, None, hdr, lens, ts)
            return snapshot(s, N)
        never = one_pass()
        assert not s.lib.DP_PortScan_Table()
        ref = s.oracle.classify_batch(hdr, lens, ts=ts, cfg=s.oracle.cfg(0, 1, 0))
        assert np.array_equal(np.array([s.mbufs[i].ppe_verdict for i in range(N)], np.uint32), ref["verdict"])
        setg(s.lib, portscan_able=1, portscan_exception_freq=3, flood_hold_time=5)
        on = one_pass()
        assert on != never and s.lib.DP_PortScan_Table()
        live = s.table()[0]["live"]
        setg(s.lib, portscan_able=0)
        assert one_pass() == never
        assert s.table()[0]["live"] == live > 0                    # the table kept its records while off
        setg(s.lib, portscan_able=2)                               # (dp_portscan.c:238: only 1 is on)
        assert one_pass() == never
    finally:
        s.close()


def test_four_threads():
    """Four threads, each with its own burst of 16, the detector on with portscan_exception_freq = 0 (every port change
    of a known source is a detection): every mbuf reaches exactly one hook, and the drop hook saw as many status-24
    packets as the table counted drops.  (Order across threads is the order in which the
    flushes take the engine: only the conservation properties are asserted.)"""
    hdr, lens, ts = scenario()
    s = Session(N)
    try:
        setg(s.lib, portscan_able=1, portscan_exception_freq=0, flood_hold_time=5)
        s.load(hdr, lens, ts)
        s.lib.Decode_Set_Burst(16)
        s.lib.DP_PortScan_Clock(*clock_at(0))
        done = []

        def worker(k):
            for i in range(k, N, 4):
                s.lib.Decode(C.byref(s.mbufs[i]))
            done.append(s.lib.Decode_Flush())
        th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join(60)
        assert len(done) == 4 and all(d >= 0 for d in done)
        assert sorted(i for i, _ in s.seen) == list(range(N))
        act = dict(s.seen)
        st = np.array([s.mbufs[i].ppe_verdict for i in range(N)], np.uint32) & 0xFF
        dropped24 = [i for i in range(N) if st[i] == ST["PORTSCAN_DROP"]]
        assert all(act[i] == 1 for i in dropped24) and not set(dropped24) & set(s.logged)
        info, _ = s.table()
        assert info["drop"] == len(dropped24) > 0
        assert info["ok"] + info["nomem"] + info["detected"] + info["hold"] == N   # every packet reached the detector
    finally:
        s.close()
