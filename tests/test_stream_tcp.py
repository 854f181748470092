"""StreamTcp's first-packet verdict, the parts that need no GPU: the tests' Python model against hand-written known
answers, `show tcpstream statistic` text against golden output generated from the reference's
dp_show_tcpstream_stat (tests/golden/gen_tcpstream_golden.py), and the additive ABI (symbols, struct sizes, the
drop-in layer's settings starting at 0)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import stream_model as sm
from ppe import abi, synth
from ppe.abi import ST

GOLDEN = Path(__file__).resolve().parent / "golden"
FW, RST, FIN, ONESIDE, MID = (ST["ACL_FW"], ST["STREAM_RST_NO_SESSION"], ST["STREAM_FIN_NO_SESSION"],
                              ST["STREAM_MIDSTREAM_ONESIDE_OFF"], ST["STREAM_MIDSTREAM_OFF"])

# (th_flags, (midstream, async_oneside), expected status): StreamTcpPacketStateNone, stream-tcp.c:243-440
KAT = [
    (0x02, (0, 0), FW),        # SYN
    (0x02, (1, 1), FW),
    (0x06, (0, 0), RST),       # SYN|RST: RST is tested first (:243)
    (0x04, (0, 0), RST),       # RST
    (0x14, (1, 0), RST),       # RST|ACK
    (0x03, (0, 0), FIN),       # SYN|FIN (:249)
    (0x01, (0, 0), FIN),       # FIN
    (0x11, (1, 1), FIN),       # FIN|ACK
    (0x07, (0, 0), RST),       # SYN|FIN|RST
    (0x12, (0, 0), ONESIDE),   # SYN|ACK under each midstream / async_oneside state (:255-261)
    (0x12, (1, 0), FW),
    (0x12, (0, 1), FW),
    (0x12, (1, 1), FW),
    (0x1A, (0, 0), ONESIDE),   # SYN|ACK|PSH
    (0x10, (0, 0), MID),       # ACK-only (:364-370)
    (0x10, (0, 1), MID),       # async_oneside does not pick up an ACK
    (0x18, (0, 0), MID),       # PSH|ACK
    (0x30, (0, 0), MID),       # URG|ACK
    (0x00, (0, 0), FW),        # no flags (:434-437)
    (0x28, (0, 0), FW),        # PSH|URG
    (0x08, (1, 1), FW),        # PSH
]


@pytest.mark.parametrize("flags,ms,want", KAT, ids=[f"{f:#04x}-m{m}a{a}" for f, (m, a), _ in KAT])
def test_model_known_answers(flags, ms, want):
    assert sm.first_packet_status(flags, *ms) == want


def test_model_ack_only_with_midstream_is_not_modelled():
    with pytest.raises(NotImplementedError):
        sm.first_packet_status(0x10, 1, 0)


def _one_packet(flags, ack, vlan=False, ihl=5):
    """A 64-B TCP frame and an oracle-shaped result saying the ACL forwarded it."""
    h = np.zeros((1, 128), np.uint8)
    l3 = 18 if vlan else 14
    h[0, l3] = 0x40 | ihl
    l4 = l3 + 4 * ihl
    h[0, l4 + 8:l4 + 12] = [(ack >> s) & 0xFF for s in (24, 16, 8, 0)]
    h[0, l4 + 13] = flags
    fl = abi.F_L4 | abi.F_TCP | abi.F_ACL | (abi.F_SYN if flags & 2 else 0) | (abi.F_VLAN if vlan else 0)
    cnt = np.zeros(32, np.uint64)
    for k in ("pkts", "l2_rx_ok", "ipv4_rx_ok", "tcp_rx_ok", "acl_fw", "flow_proc_ok", "out_fw"):
        cnt[abi.COUNTERS.index(k)] = 1
    ref = dict(verdict=np.array([FW | (fl << 16)], np.uint32), flow_hash=np.array([7], np.uint32),
               acl_hit=np.array([3], np.int32), tuple=np.zeros((1, 4), np.uint32), counters=cnt)
    return h, ref, fl


@pytest.mark.parametrize("vlan,ihl", [(False, 5), (True, 5), (False, 6), (True, 15)])
def test_model_locates_flags_and_ack(vlan, ihl):
    h, ref, fl = _one_packet(0x12, 0, vlan, ihl)
    e = sm.expected(ref, h, dict(track=1))
    assert e["verdict"][0] == ONESIDE | (abi.ACT_DROP << 8) | (fl << 16)  # flags, ACL hit, hash: the ACL's
    assert e["acl_hit"][0] == 3 and e["flow_hash"][0] == 7
    assert e["stream"] == dict(syn_ack_count=1, syn_count=0, rst_count=0, rst_but_no_session=0, fin_but_no_session=0,
                               midstream_or_oneside_disable=1, midstream_disable=0, pkt_broken_ack=0)
    c = e["counters"]
    assert (c["acl_fw"], c["flow_proc_ok"], c["flow_proc_fail"], c["out_fw"], c["out_drop"]) == (1, 1, 0, 0, 1)
    # broken ack: ACK clear, ack field non-zero (stream-tcp.c:3000); RST counted, then dropped
    h, ref, fl = _one_packet(0x06, 0x01020304, vlan, ihl)
    e = sm.expected(ref, h, dict(track=1))
    assert e["verdict"][0] & 0xFF == RST
    assert (e["stream"]["syn_count"], e["stream"]["rst_count"], e["stream"]["pkt_broken_ack"],
            e["stream"]["rst_but_no_session"]) == (1, 1, 1, 1)
    # tracking off: the oracle's answer, nothing counted
    e = sm.expected(ref, h, sm.OFF)
    assert np.array_equal(e["verdict"], ref["verdict"]) and not any(e["stream"].values())
    assert e["counters"]["out_fw"] == 1


def test_model_leaves_other_packets_alone():
    h, ref, fl = _one_packet(0x04, 5)
    for st, f in ((ST["ACL_DROP"], fl), (ST["FLOW_TCP_NO_SYN_FIRST"], fl & ~abi.F_ACL), (FW, fl & ~abi.F_TCP),
                  (ST["TCP_LEN_ERR"], 0), (ST["WINDOW_PUNT"], 0)):
        r = dict(ref, verdict=np.array([st | (f << 16)], np.uint32))
        e = sm.expected(r, h, dict(track=1))
        assert np.array_equal(e["verdict"], r["verdict"]) and not any(e["stream"].values()), st


def test_flag_sweep_generator():
    rules = synth.make_rules(256, seed=256)
    pk = synth.make_tcp_flag_sweep(rules, stride=128)
    n = len(pk["len"])
    assert n == 613 and n % 64 == 37 and pk["hdr"].shape == (n, 128)
    sw = pk["layout"] >= 0
    for lay in range(3):
        for ack in (0, 0x01020304):
            m = sw & (pk["layout"] == lay) & (pk["th_ack"] == ack) & (np.arange(n) < 512)
            assert sorted(pk["th_flags"][m]) == list(range(64))
    # the model's byte arithmetic finds the generator's fields in every layout
    fl = np.where(pk["layout"] == 1, abi.F_VLAN, 0).astype(np.uint32)
    flags, ack = sm.th_fields(pk["hdr"], fl << 16)
    assert np.array_equal(flags[sw], pk["th_flags"][sw].astype(np.uint32))
    assert np.array_equal(ack[sw], pk["th_ack"][sw])
    big = synth.make_tcp_flag_sweep(rules, stride=64, repeat=4)
    assert len(big["len"]) == 2048 + 101 and big["hdr"].shape[1] == 64
    again = synth.make_tcp_flag_sweep(rules, stride=128)
    assert np.array_equal(again["hdr"], pk["hdr"])


def _stream_counters():
    sc = abi.StreamCounters()
    for i in range(len(abi.STREAM_COUNTERS)):
        sc.c[i] = 3000 + 29 * i  # the generator's counter vector
    return sc


def test_tcpstream_stat_text_matches_reference_layout():
    lib = abi.load()
    sc = _stream_counters()
    cfg = abi.StreamTcpCfg(1, 0, 0, 0)  # the generator's setting: track enabled, reasm disabled
    n = lib.ppe_format_tcpstream_stat(C.byref(sc), C.byref(cfg), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert lib.ppe_format_tcpstream_stat(C.byref(sc), C.byref(cfg), buf, n + 1) == n
    assert buf.value.decode() == (GOLDEN / "tcpstream_stat_v1.txt").read_text()
    small = C.create_string_buffer(40)  # truncation keeps snprintf semantics
    assert lib.ppe_format_tcpstream_stat(C.byref(sc), C.byref(cfg), small, 40) == n and len(small.value) == 39
    # the enable / disable lines follow track and reasm; no setting: both disabled
    on = abi.StreamTcpCfg(0, 0, 0, 1)
    lib.ppe_format_tcpstream_stat(C.byref(sc), C.byref(on), buf, n + 1)
    assert "tcpstream track: disable\ntcpstream reasm: enable\n" in buf.value.decode()
    lib.ppe_format_tcpstream_stat(C.byref(sc), None, buf, n + 1)
    assert "tcpstream track: disable\ntcpstream reasm: disable\n" in buf.value.decode()
    assert lib.ppe_format_tcpstream_stat(None, C.byref(cfg), buf, n + 1) == abi.PPE_EINVAL


def test_additive_abi():
    lib = abi.load()
    assert lib.ppe_abi_version() == 8
    for name in ("ppe_stream_tcp_set", "ppe_stream_tcp_get", "ppe_stream_counters_read", "ppe_stream_counters_clear",
                 "ppe_format_tcpstream_stat"):
        assert hasattr(lib, name) and name in abi.EXPORTS, name
    assert C.sizeof(abi.StreamTcpCfg) == 16 and C.sizeof(abi.StreamCounters) == 128
    assert len(abi.STREAM_COUNTERS) == 8
    assert [abi.ST_NAME[s] for s in (20, 21, 22, 23)] == ["STREAM_RST_NO_SESSION", "STREAM_FIN_NO_SESSION",
                                                         "STREAM_MIDSTREAM_ONESIDE_OFF", "STREAM_MIDSTREAM_OFF"]
    # the drop-in layer's settings exist and start at 0: tracking is off until set (the reference starts it on)
    for name in ("stream_tcp_track_enable", "stream_tcp_midstream", "stream_tcp_async_oneside"):
        assert name in abi.EXPORTED_DATA
        assert C.c_uint32.in_dll(lib, name).value == 0, name


def test_header_constants_match_binding():
    """include/ppe_hip.h's new enum values and the binding's agree (compiled with gcc)."""
    import subprocess
    import tempfile
    root = Path(__file__).resolve().parent.parent
    with tempfile.TemporaryDirectory() as td:
        src = Path(td) / "k.c"
        src.write_text('#include <stdio.h>\n#include "ppe_hip.h"\nint main(void){printf("%d %d %d %d %d %d %zu %zu\\n",'
                       "PPE_ST_STREAM_RST_NO_SESSION, PPE_ST_STREAM_FIN_NO_SESSION, "
                       "PPE_ST_STREAM_MIDSTREAM_ONESIDE_OFF, PPE_ST_STREAM_MIDSTREAM_OFF, PPE_ST__COUNT, PPE_SC__COUNT, "
                       "sizeof(ppe_stream_tcp_cfg_t), sizeof(ppe_stream_counters_t));return 0;}\n")
        exe = Path(td) / "k"
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{root / 'include'}", str(src), "-o", str(exe)],
                       check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [20, 21, 22, 23, 24, 8, 16, 128]
    assert [abi.STREAM_COUNTERS.index(k) for k in ("syn_ack_count", "rst_but_no_session", "pkt_broken_ack")] == [0, 3, 7]
