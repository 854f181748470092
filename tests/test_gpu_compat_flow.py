"""The flow table behind Decode (include/ppe_decode.h: flow_able, flow_item_num, DP_Flow_Clock / DP_Flow_Age) on the GPU:
a connection's three packets at the default burst 1, repeated flows through Decode at bursts of 7, 64 and 4,096 against
the oracle's sequential FlowHandlePacket, the mbuf fields, aging, pool exhaustion, the refused combinations, release
and four threads.  Integer work: no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from mbuf_corpus import corpus, windows  # noqa: E402
from pktbuild import tcp_packet, udp_packet  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402
from pyoracle import M_FLOW  # noqa: E402
from test_gpu_compat import ALERT, HOOK, LOGGED, Mbuf, unhook  # noqa: E402
from test_gpu_flow import table  # noqa: E402
from test_gpu_mbuf import check_mbuf, new_mbufs  # noqa: E402

NOW = 1_000_000
PKT_TO_SERVER, PKT_TO_CLIENT, PKT_HAS_FLOW = 1 << 4, 1 << 5, 1 << 8
DIR = PKT_TO_SERVER | PKT_TO_CLIENT | PKT_HAS_FLOW
GLOBALS = dict(flow_able=0, flow_item_num=100000, portscan_able=0, stream_tcp_track_enable=0)
W = 144  # Decode's header window
FW, DROP = 0, 1


def setg(lib, **kw):
    for k, v in kw.items():
        C.c_uint32.in_dll(lib, k).value = v


def web_rules():
    """TCP or UDP to port 80 forwards (rule 0); everything else takes the default action, DROP."""
    r = np.zeros(1, abi.RULE_DTYPE)
    r["sport_end"] = 65535
    r["protocol_end"] = 255
    r["dport_start"], r["dport_end"] = 80, 80
    r["action"] = abi.ACL_RULE_ACTION_FW
    return r


class Session:
    """The compat layer with `rules` committed and hooks that record (mbuf index, hook); leaves the library as it found
    it (globals, hooks, burst, no context)."""

    def __init__(self, rules, default_action=DROP):
        self.lib = lib = abi.load()
        lib.ppe_set_output_hooks.argtypes = [HOOK, HOOK, HOOK]
        lib.reg_fw_alert.argtypes = [ALERT]
        self.rules, self.default_action = rules, default_action
        self.dflt = C.c_uint32.in_dll(lib, "dp_acl_action_default")
        self.old_default = self.dflt.value
        self.seen, self.logged, self.lock = [], [], threading.Lock()
        self.commit()
        self.oracle = pyoracle.Oracle(rules, default_action=default_action)

        def hook(a):
            def f(m):
                with self.lock:
                    self.seen.append(((C.addressof(m.contents) - self.base) // C.sizeof(Mbuf), a))
            return HOOK(f)
        self.hooks = [hook(a) for a in (0, 1, 2)]
        self.alert = ALERT(lambda p: self.logged.append((p - self.base) // C.sizeof(Mbuf)) or 0)
        lib.ppe_set_output_hooks(*self.hooks)
        lib.reg_fw_alert(self.alert)

    def commit(self):
        lib = self.lib
        assert lib.DP_Acl_Rule_Init() == 0
        lib.ppe_rule_list_free()
        assert lib.ppe_rule_list_init() == 0
        for i in range(len(self.rules)):
            rid = C.c_uint32()
            assert lib.Rule_add(self.rules[i:i + 1].ctypes.data, C.byref(rid)) == 0
        self.dflt.value = self.default_action
        assert lib.DP_Acl_Rule_Commit() == 0

    def load(self, hdr, lens, mbufs=None):
        n = len(lens)
        self.bufs = [C.create_string_buffer(bytes(hdr[i]), W) for i in range(n)]
        self.mbufs = mbufs if mbufs is not None else (Mbuf * n)()
        self.base = C.addressof(self.mbufs)
        for i in range(n):
            self.mbufs[i].pkt_ptr = C.cast(self.bufs[i], C.c_void_p).value
            self.mbufs[i].pkt_totallen = int(lens[i])
        del self.seen[:], self.logged[:]

    def decode(self, lo, hi):
        for i in range(lo, hi):
            self.lib.Decode(C.byref(self.mbufs[i]))

    def engine(self):
        """The shim's context as an Engine (for flow_info / flow_dump); not owned."""
        e = Engine.__new__(Engine)
        e.lib, e.ctx = self.lib, C.c_void_p(self.lib.ppe_compat_ctx())
        assert e.ctx
        return e

    def close(self):
        setg(self.lib, **GLOBALS)
        self.lib.DP_Flow_Clock(0)
        self.lib.Decode_Set_Burst(1)
        unhook(self.lib)
        self.lib.ppe_rule_list_free()
        self.lib.DP_Acl_Rule_Release()
        self.dflt.value = self.old_default


def frames_to_windows(frames):
    return windows(frames, W)


def connection():
    """SYN c->s, SYN|ACK s->c, ACK c->s of one connection to port 80."""
    c, s = 0x0A000001, 0x0A000002
    return frames_to_windows([tcp_packet(c, s, 40000, 80, flags=0x02), tcp_packet(s, c, 80, 40000, flags=0x12),
                              tcp_packet(c, s, 40000, 80, flags=0x10)])


def got(s, n):
    v = np.array([s.mbufs[i].ppe_verdict for i in range(n)], np.uint32)
    hit = np.array([s.mbufs[i].ppe_acl_hit for i in range(n)], np.int32)
    fl = np.array([s.mbufs[i].flags for i in range(n)], np.uint32)
    return v, hit, fl


def expected_flags(verdict):
    f = verdict >> 16
    return np.where(f & abi.F_FLOW, PKT_HAS_FLOW | np.where(f & abi.F_TOCLIENT, PKT_TO_CLIENT, PKT_TO_SERVER), 0)


def check_delivery(s, ref, n):
    """Every mbuf's hook, verdict, flags and hit against the oracle's outputs for the same packets in order."""
    assert sorted(i for i, _ in s.seen) == list(range(n)), "every mbuf reaches exactly one hook"
    v, hit, fl = got(s, n)
    assert np.array_equal(v, ref["verdict"]), np.flatnonzero(v != ref["verdict"])[:8]
    assert np.array_equal(hit, ref["acl_hit"])
    act = dict(s.seen)
    assert [act[i] for i in range(n)] == ((ref["verdict"] >> 8) & 0xFF).tolist()
    assert np.array_equal(fl & DIR, expected_flags(ref["verdict"]))
    st = ref["verdict"] & 0xFF
    assert sorted(s.logged) == np.flatnonzero(np.isin(st, list(LOGGED))).tolist()      # FLOW_NOMEM is not among them


def test_connection_known_answer_at_burst_one():
    hdr, lens = connection()
    s = Session(web_rules())
    try:
        # flow_able = 0 is the stateless Decode: every packet its flow's first.  The SYN forwards by rule 0; the
        # SYN|ACK carries SYN (TCP_IS_SYN, decode-tcp.h:90), passes syn_check and meets the ACL as a first packet: no
        # rule, default DROP; the ACK is dropped as FLOW_TCP_NO_SYN_FIRST
        s.load(hdr, lens)
        s.decode(0, 3)
        v, hit, fl = got(s, 3)
        assert (v & 0xFF).tolist() == [ST["ACL_FW"], ST["ACL_DROP"], ST["FLOW_TCP_NO_SYN_FIRST"]]
        assert s.seen == [(0, FW), (1, DROP), (2, DROP)] and hit.tolist() == [0, -1, -1]
        assert (fl & DIR).tolist() == [PKT_TO_SERVER | PKT_HAS_FLOW, 0, 0]
        ref = s.oracle.classify_batch(hdr, lens, cfg=s.oracle.cfg(0, 1, 0))
        assert np.array_equal(v, ref["verdict"])
        # flow_able = 1: the SYN creates the flow, the reply and the ACK find it (no ACL lookup)
        setg(s.lib, flow_able=1)
        s.lib.DP_Flow_Clock(NOW)
        s.load(hdr, lens)
        for i in range(3):
            s.decode(i, i + 1)
            assert s.seen[-1] == (i, FW), "delivered before Decode returns"
        v, hit, fl = got(s, 3)
        assert (v & 0xFF).tolist() == [ST["ACL_FW"]] * 3 and hit.tolist() == [0, -1, -1]
        assert (fl & DIR).tolist() == [PKT_TO_SERVER | PKT_HAS_FLOW, PKT_TO_CLIENT | PKT_HAS_FLOW,
                                       PKT_TO_SERVER | PKT_HAS_FLOW]
        assert (v[0] >> 16) & abi.F_NEWFLOW and not ((v[1] | v[2]) >> 16) & (abi.F_NEWFLOW | abi.F_ACL)
        d = s.engine().flow_dump()
        assert len(d) == 1 and (int(d["pktcnts2d"][0]), int(d["pktcntd2s"][0])) == (2, 1)
        assert int(d["last_seen"][0]) == NOW and (int(d["sport"][0]), int(d["dport"][0])) == (40000, 80)
        # off again: today's answers, and the table keeps its flow
        setg(s.lib, flow_able=0)
        s.load(hdr, lens)
        s.decode(0, 3)
        assert (got(s, 3)[0] & 0xFF).tolist() == [ST["ACL_FW"], ST["ACL_DROP"], ST["FLOW_TCP_NO_SYN_FIRST"]]
        assert s.engine().flow_info()["live"] == 1
    finally:
        s.close()


_flow_case = {}


def flow_case():
    """5,000 packets over 600 flows in both directions (a third of the TCP packets SYN), 144-B windows, with the
    oracle's whole-batch answer: the flow path is sequential, so every burst size must give exactly this."""
    if not _flow_case:
        rules = synth.make_rules(256, seed=21)
        pk = synth.make_flow_packets(5000, rules, n_flows=600, seed=77, kind="imix", stride=128, malformed_frac=0.01)
        hdr = np.zeros((5000, W), np.uint8)
        hdr[:, :128] = pk["hdr"]
        o = pyoracle.Oracle(rules, default_action=FW)
        ft = pyoracle.OracleFlow(o, capacity=100000)
        ref = ft.classify_batch(hdr, pk["len"], ts=np.zeros(5000, np.uint64), cfg=o.cfg(0, 1, NOW))
        _flow_case.update(rules=rules, hdr=hdr, lens=pk["len"], ref=ref, table=table(ft.dump()), stats=ft.stats())
        ft.close()
    return _flow_case


@pytest.mark.parametrize("burst", [7, 64, 4096])
def test_bursts_over_repeated_flows(burst):
    c = flow_case()
    n = len(c["lens"])
    s = Session(c["rules"], default_action=FW)
    try:
        setg(s.lib, flow_able=1)
        s.lib.DP_Flow_Clock(NOW)
        s.lib.Decode_Set_Burst(burst)
        s.load(c["hdr"], c["lens"])
        s.decode(0, n)
        assert s.lib.Decode_Flush() == n % burst
        check_delivery(s, c["ref"], n)
        f = c["ref"]["verdict"] >> 16
        assert (f & abi.F_TOCLIENT).any() and (f & abi.F_NEWFLOW).any() and ((f & abi.F_FLOW) == 0).any()
        e = s.engine()
        assert table(e.flow_dump()) == c["table"]
        info = e.flow_info()
        assert (info["live"], info["new_flow"], info["del_flow"]) == tuple(c["stats"][k] for k in
                                                                          ("live", "new_flow", "del_flow"))
        assert info["capacity"] == 100000 and info["max_batch"] == 4096   # (a 4,096 burst fits; none is larger)
    finally:
        s.close()


def test_mbuf_fields_with_the_table_on():
    """The mbuf field corpus through Decode with the flow table on: every decoder field as with it off (the oracle's
    record of the whole frame), the flow flags from the flow oracle's verdict, m->flow untouched."""
    frames, kinds = corpus(3000, seed=41)
    n = len(frames)
    rules = synth.make_rules(300, seed=44)
    hdr, lens = windows(frames, W)
    s = Session(rules, default_action=FW)
    try:
        setg(s.lib, flow_able=1)
        s.lib.Decode_Set_Burst(1000)
        bufs = [C.create_string_buffer(f, max(len(f), 1)) for f in frames]
        mb = new_mbufs(frames, bufs)
        s.mbufs, s.base = mb, C.addressof(mb)
        del s.seen[:], s.logged[:]
        s.decode(0, n)
        assert s.lib.Decode_Flush() == 0 and sorted(i for i, _ in s.seen) == list(range(n))
        ft = pyoracle.OracleFlow(s.oracle, capacity=100000)
        ref = ft.classify_batch(hdr, lens, ts=np.zeros(n, np.uint64), cfg=s.oracle.cfg(0, 1, 0))
        ft.close()
        v = np.array([mb[i].ppe_verdict for i in range(n)], np.uint32)
        assert np.array_equal(v, ref["verdict"]), np.flatnonzero(v != ref["verdict"])[:8]
        want = expected_flags(ref["verdict"])
        cfg = s.oracle.cfg(0, 1, 0)
        for i in range(n):
            f = frames[i]
            buf = np.frombuffer(f, np.uint8).copy() if f else np.zeros(1, np.uint8)
            r = pyoracle.OResult()
            s.oracle.lib.oracle_classify(buf.ctypes.data, len(f), len(f), 0, C.byref(cfg), C.byref(r))
            r = {k: getattr(r, k) for k, _ in pyoracle.OResult._fields_}
            assert mb[i].flags == want[i], (i, kinds[i], mb[i].flags, int(want[i]))
            # the decoders' fields do not depend on the table: test_gpu_mbuf's check with the stateless flow flags
            mb[i].flags = (PKT_TO_SERVER | PKT_HAS_FLOW) if r["mset"] & M_FLOW else 0
            try:
                check_mbuf(mb[i], r, f, C.cast(bufs[i], C.c_void_p).value)
            except AssertionError as e:
                raise AssertionError(f"packet {i} ({kinds[i]}, status {r['status']}, mset {r['mset']:#x})") from e
    finally:
        s.close()


def test_clock_and_age_at_the_strict_boundary():
    """Flows last seen at NOW and at NOW + 5: DP_Flow_Age at NOW + 20 deletes none (now - last > 20 is strict), at
    NOW + 21 exactly the first group, as the oracle."""
    c = flow_case()
    s = Session(c["rules"], default_action=FW)
    o = pyoracle.Oracle(c["rules"], default_action=FW)
    ft = pyoracle.OracleFlow(o, capacity=100000)
    try:
        setg(s.lib, flow_able=1)
        s.lib.Decode_Set_Burst(500)
        s.load(c["hdr"][:1000], c["lens"][:1000])
        for k, (lo, hi) in enumerate(((0, 500), (500, 1000))):
            s.lib.DP_Flow_Clock(NOW + 5 * k)
            s.decode(lo, hi)
            ft.classify_batch(c["hdr"][lo:hi], c["lens"][lo:hi], ts=np.zeros(hi - lo, np.uint64), cfg=o.cfg(0, 1, NOW + 5 * k))
        e = s.engine()
        assert table(e.flow_dump()) == table(ft.dump())
        last = e.flow_dump()["last_seen"]
        assert (last == NOW).any() and (last == NOW + 5).any()
        deleted = C.c_uint64(99)
        assert s.lib.DP_Flow_Age(NOW + 20, C.byref(deleted)) == 0 and deleted.value == ft.age(NOW + 20) == 0
        assert s.lib.DP_Flow_Age(NOW + 21, C.byref(deleted)) == 0
        assert deleted.value == ft.age(NOW + 21) == int((last == NOW).sum())
        assert table(e.flow_dump()) == table(ft.dump())
        assert s.lib.DP_Flow_Age(NOW + 21, None) == 0
    finally:
        ft.close()
        s.close()


def test_small_pool_gives_flow_nomem_through_the_drop_hook():
    n = 40
    hdr, lens = frames_to_windows([udp_packet(0x0A000100 + i, 0x0A000002, 5000 + i, 80) for i in range(n)])
    s = Session(web_rules())
    ft = None
    try:
        setg(s.lib, flow_able=1, flow_item_num=8)
        s.lib.Decode_Set_Burst(16)
        s.load(hdr, lens)
        s.decode(0, n)
        assert s.lib.Decode_Flush() == n % 16
        ft = pyoracle.OracleFlow(s.oracle, capacity=8)
        ref = ft.classify_batch(hdr, lens, ts=np.zeros(n, np.uint64), cfg=s.oracle.cfg(0, 1, 0))
        check_delivery(s, ref, n)
        st = ref["verdict"] & 0xFF
        assert (st[:8] == ST["ACL_FW"]).all() and (st[8:] == ST["FLOW_NOMEM"]).all()
        act = dict(s.seen)
        assert all(act[i] == DROP for i in range(8, n)) and not s.logged          # flow.c:124-129 logs nothing
        assert (got(s, n)[2][8:] & DIR == 0).all()
        info = s.engine().flow_info()
        assert info["live"] == 8 and info["capacity"] == 8
    finally:
        if ft:
            ft.close()
        s.close()


@pytest.mark.parametrize("other", ["portscan_able", "stream_tcp_track_enable"])
def test_refused_combinations_drop_the_burst_and_change_nothing(other):
    hdr, lens = connection()
    s = Session(web_rules())
    try:
        setg(s.lib, flow_able=1)
        s.lib.DP_Flow_Clock(NOW)
        s.load(hdr[:1], lens[:1])
        s.decode(0, 1)                                              # the SYN: one flow
        e = s.engine()
        before = (table(e.flow_dump()), e.flow_info())
        setg(s.lib, **{other: 1})
        s.lib.Decode_Set_Burst(8)
        s.load(hdr, lens)
        s.decode(0, 3)
        assert s.lib.Decode_Flush() == abi.PPE_ENOTSUP
        assert sorted(s.seen) == [(0, DROP), (1, DROP), (2, DROP)]   # every mbuf, the drop hook, exactly once
        assert (table(e.flow_dump()), e.flow_info()) == before
        assert not s.lib.DP_PortScan_Table()
        setg(s.lib, **{other: 0})                                   # and the table goes on where it was
        s.load(hdr, lens)
        s.decode(0, 3)
        assert s.lib.Decode_Flush() == 3 and [a for _, a in sorted(s.seen)] == [FW, FW, FW]
    finally:
        s.close()


def test_release_then_a_fresh_table():
    hdr, lens = connection()
    s = Session(web_rules())
    try:
        setg(s.lib, flow_able=1)
        s.load(hdr, lens)
        s.decode(0, 3)
        assert s.engine().flow_info()["new_flow"] == 1
        s.lib.DP_Acl_Rule_Release()
        deleted = C.c_uint64(5)
        assert s.lib.DP_Flow_Age(NOW, C.byref(deleted)) == 0 and deleted.value == 0      # no context, no table
        s.commit()
        s.load(hdr[2:], lens[2:])                                   # the ACK alone: its flow is gone
        s.decode(0, 1)
        assert s.mbufs[0].ppe_verdict & 0xFF == ST["FLOW_TCP_NO_SYN_FIRST"] and s.seen == [(0, DROP)]
        info = s.engine().flow_info()
        assert (info["live"], info["new_flow"]) == (0, 0)
    finally:
        s.close()


def test_four_threads_disjoint_flows():
    """Four threads each Decode their own connections at burst 1 (SYN, SYN|ACK, ACK per connection, in order): every
    mbuf reaches exactly one hook with the verdict of its thread's own sequence (the flows are disjoint, so the
    order across threads does not matter), and the table holds one flow per connection."""
    per, T = 20, 4
    fr = []
    for t in range(T):
        for k in range(per):
            c, srv, sp = 0x0A010000 + (t << 8) + k, 0x0A000002, 30000 + k
            fr += [tcp_packet(c, srv, sp, 80, flags=0x02), tcp_packet(srv, c, 80, sp, flags=0x12),
                   tcp_packet(c, srv, sp, 80, flags=0x10)]
    hdr, lens = frames_to_windows(fr)
    n = len(lens)
    s = Session(web_rules())
    try:
        setg(s.lib, flow_able=1)
        s.lib.DP_Flow_Clock(NOW)
        s.lib.Decode_Set_Burst(1)
        s.load(hdr, lens)

        def worker(t):
            s.decode(3 * per * t, 3 * per * (t + 1))
        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join(60)
        assert not any(x.is_alive() for x in th)
        ft = pyoracle.OracleFlow(s.oracle, capacity=100000)
        ref = ft.classify_batch(hdr, lens, ts=np.zeros(n, np.uint64), cfg=s.oracle.cfg(0, 1, NOW))
        check_delivery(s, ref, n)
        order = [i for i, _ in s.seen]
        for t in range(T):                                          # per-thread order is kept
            mine = [i for i in order if 3 * per * t <= i < 3 * per * (t + 1)]
            assert mine == sorted(mine)
        e = s.engine()
        assert e.flow_info()["live"] == T * per == int(((ref["verdict"] >> 16) & abi.F_NEWFLOW != 0).sum())
        assert table(e.flow_dump()) == table(ft.dump())
        ft.close()
    finally:
        s.close()
