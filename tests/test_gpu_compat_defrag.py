"""Reassembly behind Decode (include/ppe_decode.h: defrag_able, defrag_cache_max, DP_Defrag_Clock / _Age / _Table) on the
GPU against the serial model of the flush (tests/compat_defrag_model.py, pinned on the CPU by
tests/test_compat_defrag_model.py): the known answers and the reassembly corpus at bursts 1, 64 and 300, the switch
with a fragment held across it, aging on the timeout's edge, a reassembled SYN through the flow table, the release with
fragments held, four threads, and the show text.

Bar: the hook sequence (with DP_Log_Func's calls) equal to the model's; every reassembled mbuf's fields, frame bytes
and fragment chain in order equal to the model's datagram; every mbuf handed to exactly one hook."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loads the HIP runtime first)

from compat_defrag_model import DecodeDefragModel  # noqa: E402
from pktbuild import ip_frag, tcp, tcp_packet, udp, udp_packet  # noqa: E402
from ppe import abi  # noqa: E402
from test_gpu_compat import ALERT, HOOK, Mbuf  # noqa: E402
from test_gpu_compat_flow import Session, setg  # noqa: E402

import defrag_corpus as dfc  # noqa: E402

S, D, NOW = 0x0A000001, 0x0A000002, 1000
PKT_FRAG_REASM_COMP, PKT_HAS_FLOW, PKT_TO_SERVER, PKT_TO_CLIENT = 1 << 3, 1 << 8, 1 << 4, 1 << 5
NAMES = {0: "fw", 1: "drop", 2: "punt"}


def web_rules():
    r = np.zeros(1, abi.RULE_DTYPE)
    r["sport_end"] = 65535
    r["protocol_end"] = 255
    r["dport_start"], r["dport_end"] = 80, 80
    r["action"] = abi.ACL_RULE_ACTION_FW
    return r


class FragSession(Session):
    """Session with whole frames behind the mbufs and hooks that record events as the model names them; a reassembled
    mbuf (not one of the caller's) is read inside the hook, where it is valid: its fields, frame and chain."""

    def __init__(self, rules, default_action=1):
        super().__init__(rules, default_action)
        self.events, self.dgrams = [], []
        size = C.sizeof(Mbuf)

        def who(addr):
            k = (addr - self.base) // size
            return k if 0 <= k < self.n and self.base + k * size == addr else None

        def hook(a):
            def f(m):
                addr = C.addressof(m.contents)
                with self.lock:
                    k = who(addr)
                    if k is None:
                        mb = m.contents
                        chain, p = [], mb.fragments
                        while p and len(chain) < 64:
                            chain.append(who(p))
                            p = Mbuf.from_address(p).next
                        self.dgrams.append(dict(
                            frame=C.string_at(mb.pkt_ptr, mb.pkt_totallen), chain=chain, verdict=mb.ppe_verdict,
                            hit=mb.ppe_acl_hit, flags=mb.flags, magic=mb.magic_flag, space=mb.pkt_space,
                            port=mb.input_port, ts=mb.timestamp, next=mb.next, flow=mb.flow, fcb=mb.fcb))
                        k = ("dgram", len(self.dgrams) - 1)
                    self.events.append((NAMES[a], k))
            return HOOK(f)

        def alert(p):
            with self.lock:
                k = who(p)
                self.events.append(("log", k if k is not None else ("dgram", len(self.dgrams))))
            return 0
        self.hooks = [hook(a) for a in (0, 1, 2)]
        self.alert = ALERT(alert)
        self.lib.ppe_set_output_hooks(*self.hooks)
        self.lib.reg_fw_alert(self.alert)

    def load_frames(self, frames, ports=None):
        self.n = n = len(frames)
        self.frames = frames
        self.bufs = [C.create_string_buffer(bytes(f), len(f) + 8) for f in frames]
        self.mbufs = (Mbuf * n)()
        self.base = C.addressof(self.mbufs)
        for i in range(n):
            self.mbufs[i].pkt_ptr = C.cast(self.bufs[i], C.c_void_p).value
            self.mbufs[i].pkt_totallen = len(frames[i])
            self.mbufs[i].input_port = ports[i] if ports else 100 + i % 7
            self.mbufs[i].timestamp = 0
        del self.events[:], self.dgrams[:]

    def run(self, burst, lo=0, hi=None):
        """Decode mbufs [lo, hi) at `burst`, with a final flush; returns that flush's count of hook calls."""
        hi = self.n if hi is None else hi
        self.lib.Decode_Set_Burst(burst)
        for i in range(lo, hi):
            self.lib.Decode(C.byref(self.mbufs[i]))
        rc = self.lib.Decode_Flush()
        assert rc >= 0
        return rc

    def close(self):
        setg(self.lib, defrag_able=0, defrag_cache_max=8)
        self.lib.DP_Defrag_Clock(0)
        super().close()


def model_events(m, frames, burst, now):
    ev = []
    for b in range(0, len(frames), burst):
        ev += m.flush(frames[b:b + burst], list(range(b, min(b + burst, len(frames)))), now)
    return ev


def check_against_model(s, m, ev):
    """s.events == the model's, datagram by datagram: who -> ("dgram", running number)."""
    want, order = [], []
    for h, who in ev:
        if isinstance(who, tuple):
            if not order or order[-1] != who[1]:
                order.append(who[1])
            who = ("dgram", len(order) - 1)
        want.append((h, who))
    assert s.events == want
    assert len(s.dgrams) == len(order)
    for got, key in zip(s.dgrams, order):
        d = m.dgrams[key]
        assert got["frame"] == d["frame"] and got["chain"] == d["chain"], key
        assert got["verdict"] == d["verdict"] and got["hit"] == d["hit"], key
        head = s.mbufs[d["chain"][0]]
        assert (got["magic"], got["space"], got["port"], got["ts"]) == (abi.MBUF_MAGIC_NUM, 2, head.input_port, 0)
        assert got["flags"] & PKT_FRAG_REASM_COMP and not got["next"] and not got["flow"] and not got["fcb"]


def halves(dport, ident=7, sip=S, proto_l4=None):
    l4 = proto_l4 if proto_l4 is not None else udp(1000, dport, bytes(range(24)))
    proto = 17 if proto_l4 is None else 6
    return ip_frag(proto, sip, D, ident, 0, True, l4[:16]), ip_frag(proto, sip, D, ident, 16, False, l4[16:])


def known_frames():
    """The model's known answers in one stream: whole packets, a datagram in order, one reversed, a teardrop, a cache
    that fills (with its log), a datagram the ACL drops."""
    f0, f1 = halves(80, 7)
    g0, g1 = halves(80, 8, S + 1)
    h0, h1 = halves(81, 9, S + 2)
    l4 = udp(1000, 80, bytes(range(24)))
    t0 = ip_frag(17, S + 3, D, 10, 0, True, l4[:16])
    t1 = ip_frag(17, S + 3, D, 10, 8, True, l4[8:24])
    full = [ip_frag(17, S + 4, D, 11, 8 * k, True, bytes(range(8))) for k in range(1, 10)]
    return [udp_packet(dport=80), f0, udp_packet(dport=81), f1, g1, g0, t0, t1, *full, h0, h1, udp_packet(dport=80)]


@pytest.mark.parametrize("burst", [1, 64, 300])
def test_known_answers(burst):
    frames = known_frames()
    s, m = FragSession(web_rules()), DecodeDefragModel(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        calls = s.run(burst)
        ev = model_events(m, frames, burst, NOW)
        check_against_model(s, m, ev)
        if burst > 1:   # one flush: Decode_Flush counts its hook calls (held fragments have none, a chain has one)
            assert calls == sum(1 for h, _ in ev if h != "log") < len(frames)
        fw = [who for h, who in s.events if h == "fw" and isinstance(who, tuple)]
        assert len(fw) == 2 and [d["chain"] for d in s.dgrams[:2]] == [[1, 3], [5, 4]]
        assert ("log", 16) in s.events and s.events.index(("log", 16)) + 1 == s.events.index(("drop", 16))
        # what is still held goes to the drop hook when the timeout passes: the same mbufs as the model's
        n0 = len(s.events)
        dropped = C.c_uint64(0)
        assert s.lib.DP_Defrag_Age(NOW + 21, C.byref(dropped)) == 0
        assert sorted(s.events[n0:]) == m.age(NOW + 21) and dropped.value == len(s.events) - n0 > 0
        seen = [who for h, who in s.events if h != "log" and not isinstance(who, tuple)]
        seen += [k for d in s.dgrams for k in d["chain"]]
        assert sorted(seen) == list(range(len(frames))), "every mbuf reaches exactly one hook, alone or in a chain"
    finally:
        s.close()
        m.close()


@pytest.mark.parametrize("burst", [1, 64, 300])
def test_corpus_through_decode(burst):
    frames = [fr[:n] for c in dfc.cases() for fr, n in c.frames]
    rules = web_rules()   # (and the default action FW: the corpus's one datagram that reaches the ACL forwards)
    s, m = FragSession(rules, default_action=0), DecodeDefragModel(rules, default_action=0)
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        s.run(burst)
        check_against_model(s, m, model_events(m, frames, burst, NOW))
        assert any(h == "fw" and isinstance(w, tuple) for h, w in s.events)
        assert any(h == "drop" and isinstance(w, tuple) for h, w in s.events)
        n0 = len(s.events)
        assert s.lib.DP_Defrag_Age(NOW + 100, None) == 0
        assert sorted(s.events[n0:]) == m.age(NOW + 100)
    finally:
        s.close()
        m.close()


def test_switch_off_and_on_with_a_fragment_held():
    f0, f1 = halves(80)
    s = FragSession(web_rules())
    try:
        s.load_frames([f0, f1, f0, f1])
        assert s.run(64, 0, 1) == 1 and s.events == [("punt", 0)]         # defrag_able 0: today's Decode
        assert not s.lib.DP_Defrag_Table()
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        assert s.run(64, 2, 3) == 0 and s.events == [("punt", 0)]         # held: no hook
        assert s.lib.DP_Defrag_Table()
        setg(s.lib, defrag_able=0)
        assert s.run(64, 1, 2) == 1 and s.events[-1] == ("punt", 1)       # off again: punted, the table untouched
        fi = abi.DefragInfo()
        assert s.lib.ppe_defrag_info(C.c_void_p(s.lib.DP_Defrag_Table()), C.byref(fi)) == 0 and fi.running == 1
        setg(s.lib, defrag_able=1)
        assert s.run(64, 3, 4) == 1                                        # the held head and this tail: one datagram
        assert s.events[-1] == ("fw", ("dgram", 0)) and s.dgrams[0]["chain"] == [2, 3]
    finally:
        s.close()


@pytest.mark.parametrize("idle,dropped", [(20, 0), (21, 1)])
def test_age_on_the_timeout(idle, dropped):
    f0, f1 = halves(80)
    s = FragSession(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames([f0, f1])
        s.run(1, 0, 1)
        n = C.c_uint64(9)
        setg(s.lib, defrag_able=0)                                         # aging works with the switch off
        assert s.lib.DP_Defrag_Age(NOW + idle, C.byref(n)) == 0 and n.value == dropped
        assert s.events == [("drop", 0)] * dropped                         # no DP_Log_Func
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW + idle)
        s.run(1, 1, 2)
        assert (s.events[-1] == ("fw", ("dgram", 0))) == (dropped == 0)
    finally:
        s.close()


def test_a_reassembled_syn_creates_the_flow_its_reply_finds():
    syn = tcp(40000, 80, flags=0x02, payload=bytes(12))
    f0, f1 = halves(80, 21, S, proto_l4=syn)
    reply = tcp_packet(D, S, 80, 40000, flags=0x12)
    s = FragSession(web_rules())
    try:
        setg(s.lib, defrag_able=1, flow_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.lib.DP_Flow_Clock(NOW)
        s.load_frames([f0, f1, reply])
        s.run(1)
        assert s.events == [("fw", ("dgram", 0)), ("fw", 2)]
        d = s.dgrams[0]
        assert d["chain"] == [0, 1] and d["hit"] == 0
        assert d["flags"] & (PKT_HAS_FLOW | PKT_TO_SERVER | PKT_FRAG_REASM_COMP) == PKT_HAS_FLOW | PKT_TO_SERVER | PKT_FRAG_REASM_COMP
        assert s.mbufs[2].flags & (PKT_HAS_FLOW | PKT_TO_CLIENT) == PKT_HAS_FLOW | PKT_TO_CLIENT
        assert s.mbufs[2].ppe_acl_hit == -1                                # found its flow: no ACL lookup
    finally:
        setg(s.lib, flow_able=0)
        s.close()


def test_release_with_fragments_held():
    heads = [halves(80, 30 + k, S + k)[0] for k in range(5)]
    s = FragSession(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.load_frames(heads)
        assert s.run(64) == 0 and s.events == []
        s.lib.DP_Acl_Rule_Release()
        assert sorted(s.events) == [("drop", k) for k in range(5)]
        assert not s.lib.DP_Defrag_Table()
        assert s.lib.DP_Defrag_Age(NOW, None) == 0
    finally:
        s.close()


def test_four_threads_over_disjoint_keys():
    per = 40
    frames = []
    for t in range(4):
        for k in range(per):
            f0, f1 = halves(80 if k % 2 == 0 else 81, 100 + k, S + 256 * (t + 1) + k)
            frames += [f0, f1]
    s = FragSession(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        s.lib.Decode_Set_Burst(16)

        def work(t):
            for i in range(2 * per * t, 2 * per * (t + 1)):
                s.lib.Decode(C.byref(s.mbufs[i]))
            s.lib.Decode_Flush()
        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert len(s.dgrams) == 4 * per
        assert sorted(tuple(d["chain"]) for d in s.dgrams) == [(2 * i, 2 * i + 1) for i in range(4 * per)]
        for d in s.dgrams:
            want = abi.ST["ACL_FW"] if (d["chain"][0] // 2) % per % 2 == 0 else abi.ST["ACL_DROP"]
            assert d["verdict"] & 0xFF == want
        fi = abi.DefragInfo()
        assert s.lib.ppe_defrag_info(C.c_void_p(s.lib.DP_Defrag_Table()), C.byref(fi)) == 0
        assert fi.datagrams == 4 * per and fi.st[abi.DF["CACHED"]] == 4 * per
    finally:
        s.close()


def test_show_text_after_a_run():
    frames = known_frames()
    s, m = FragSession(web_rules()), DecodeDefragModel(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        s.run(64)
        model_events(m, frames, 64, NOW)
        gi, oi, os_ = abi.DefragInfo(), abi.DefragInfo(), m.d.stats()
        assert s.lib.ppe_defrag_info(C.c_void_p(s.lib.DP_Defrag_Table()), C.byref(gi)) == 0
        for k in range(9):
            oi.st[k] = os_["st_" + abi.DF_NAME[k].lower()]
        oi.teardrop, oi.new_fcb, oi.del_fcb = os_["teardrop"], os_["new_fcb"], os_["del_fcb"]
        cnt, fl, texts = abi.Counters(), abi.FlowInfo(), []
        for info in (gi, oi):
            buf, fbuf = C.create_string_buffer(8192), C.create_string_buffer(512)
            s.lib.ppe_format_pkt_stat_ex(C.byref(cnt), C.byref(info), 1, buf, 8192)
            s.lib.ppe_format_flow_stat_ex(C.byref(fl), C.byref(info), fbuf, 512)
            texts.append((buf.value.decode(), fbuf.value.decode()))
        assert texts[0] == texts[1]
        assert f"reasm_ok: {oi.st[abi.DF['REASM']]}\n" in texts[0][0] and oi.st[abi.DF["REASM"]] == 3
    finally:
        s.close()
        m.close()


def test_fcb_full_goes_to_the_drop_hook():
    """1,030 first fragments of different datagrams at burst 300: the table has DEFRAG_FCB_MAX = 1,024 FCBs, the last
    six fragments go to the drop hook without a log; the model's events, then everything held by the release."""
    l4 = udp(1000, 80, bytes(range(24)))
    frames = [ip_frag(17, S + 16 + k, D, 500, 0, True, l4[:16]) for k in range(1030)]
    s, m = FragSession(web_rules()), DecodeDefragModel(web_rules())
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        s.run(300)
        ev = model_events(m, frames, 300, NOW)
        assert ev == [("drop", k) for k in range(1024, 1030)]
        check_against_model(s, m, ev)
        fi = abi.DefragInfo()
        assert s.lib.ppe_defrag_info(C.c_void_p(s.lib.DP_Defrag_Table()), C.byref(fi)) == 0
        assert fi.st[abi.DF["FCB_FULL"]] == 6 and fi.running == 1024
        s.lib.DP_Acl_Rule_Release()
        assert sorted(s.events) == [("drop", k) for k in range(1030)]
    finally:
        s.close()
        m.close()


@pytest.mark.parametrize("step", [1, 2])
def test_a_failed_step_drops_every_mbuf_once(step):
    """The defrag step (1) or the datagrams' classify step (2) fails (the shim's test hook): every mbuf of the burst
    and everything the table held reach the drop hook exactly once, nothing else is called, the table is gone, and the
    next flush starts a fresh one.  The burst has a whole packet, a fragment that is cached (held by this burst), a
    tail that completes a datagram whose head an earlier burst left in the table, and a datagram whose head and tail
    both lie in it (the head is cached, then taken by the chain its tail completes); another earlier head stays held."""
    f0, f1 = halves(80, 7)
    g0, _ = halves(80, 8, S + 1)
    h0, _ = halves(80, 9, S + 2)
    k0, k1 = halves(80, 10, S + 3)
    frames = [f0, g0, udp_packet(dport=80), h0, f1, f0, f1, k0, k1]
    s = FragSession(web_rules())
    s.lib.ppe_compat_debug_fail_defrag_step.argtypes = [C.c_uint32]
    s.lib.ppe_compat_debug_fail_defrag_step.restype = None
    try:
        setg(s.lib, defrag_able=1)
        s.lib.DP_Defrag_Clock(NOW)
        s.load_frames(frames)
        assert s.run(64, 0, 2) == 0 and s.events == []          # two heads held by an earlier burst
        s.lib.ppe_compat_debug_fail_defrag_step(step)
        s.lib.Decode_Set_Burst(64)
        for i in (2, 3, 7, 4, 8):
            s.lib.Decode(C.byref(s.mbufs[i]))
        assert s.lib.Decode_Flush() == -5                        # PPE_EIO
        assert sorted(s.events) == [("drop", k) for k in (0, 1, 2, 3, 4, 7, 8)], "each mbuf once, through the drop hook"
        assert not s.dgrams and not s.lib.DP_Defrag_Table()
        n0 = len(s.events)
        assert s.run(64, 5, 7) == 1                              # a fresh table: the datagram again, from new mbufs
        assert s.events[n0:] == [("fw", ("dgram", 0))] and s.dgrams[0]["chain"] == [5, 6]
        assert s.lib.DP_Defrag_Age(NOW + 100, None) == 0 and len(s.events) == n0 + 1
    finally:
        s.lib.ppe_compat_debug_fail_defrag_step(0)
        s.close()
