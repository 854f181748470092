"""The land, SYN-flood and UDP-flood monitors (ppe_attack_*) on the CPU: hand-derived known answers of the tests' serial
model (tests/attack_model.py) over the CPU oracle, the frozen scenario, the two show texts against text restated from
the reference's sprintf calls, the binding against the header, and the host-only planner entry.

dp_attack.c includes the Cavium headers and does not build on a PC, so nothing here is pinned by reference outputs:
the model is a line-cited restatement, and these are the answers worked out by hand from the cited lines."""
import ctypes as C
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

import attack_model as am
import pyoracle
from attack_model import AttackModel, batch, frame
from portscan_model import PortScanModel
from ppe import abi
from ppe.abi import ST

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NOW = 1_700_000_000
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
FW = ST["ACL_FW"]
A, B = 0x0A000001, 0x0B000002


def oracle():
    return pyoracle.Oracle(None, default_action=abi.ACL_RULE_ACTION_FW)


def run(m, frames, ports=None, o=None, syn_check=1, **kw):
    """Statuses of one batch through the oracle and the model; the full result under run.last."""
    o = o or oracle()
    hdr, lens = batch(frames)
    ref = o.classify_batch(hdr, lens, cfg=o.cfg(0, syn_check, NOW))
    run.last = e = m.expected(ref, hdr, ports, **kw)
    run.ref = ref
    return (e["verdict"] & 0xFF).tolist()


def test_enable_fields_compare_with_one():
    """Every enable field at 0 / 1 / 2 and drop_pack at 0 / 1 / 2 on both rule halves: only 1 acts (ATTACK_ENABLE)."""
    for v in (0, 1, 2):
        for dp in (0, 1, 2):
            on = v == 1 and dp == 1
            m = AttackModel({0: dict(land=v, drop_pack=dp)})
            assert run(m, [frame("syn", A, A)]) == [LAND if on else FW]
            assert m.info()["land_drop"] == int(on) and m.ai[0]["syn_accum"] == int(not on)
            m = AttackModel(td={0: dict(flood_udp=v, udp_speed=0, drop_pack=dp)})
            m.ai[0]["udppps"] = 1
            assert run(m, [frame("udp")] * 2) == [UDPF if on else FW] * 2
            assert m.ai[0]["udp_flood_hold"] == int(on) and m.ai[0]["udp_accum"] == 2
            m = AttackModel(td={0: dict(flood_syn=v, syn_speed=0, syn_count=9, drop_pack=dp)})
            m.ai[0]["synpps"] = 1
            assert run(m, [frame("syn")] * 2) == [SYNF if on else FW] * 2
            assert m.ai[0]["syn_flood_hold"] == int(on) and m.ai[0]["syn_accum"] == 2
    # the packet-detect half's drop_pack does not stand in for the traffic half's, and the other way round
    m = AttackModel({0: dict(land=1, drop_pack=0)}, {0: dict(drop_pack=1)})
    assert run(m, [frame("syn", A, A)]) == [FW]
    m = AttackModel({0: dict(drop_pack=1)}, {0: dict(flood_udp=1, drop_pack=0)})
    m.ai[0]["udppps"] = 5
    assert run(m, [frame("udp")]) == [FW]


def test_speed_thresholds_are_strict():
    """pps == speed passes, speed + 1 drops (uint64 > uint32); syncount == syn_count passes, + 1 drops, and drops with
    flood_syn 0."""
    for pps, want in ((7, FW), (8, UDPF)):
        m = AttackModel(td={0: dict(flood_udp=1, udp_speed=7, drop_pack=1)})
        m.ai[0]["udppps"] = pps
        assert run(m, [frame("udp")]) == [want]
    for pps, want in ((7, FW), (8, SYNF), ((1 << 32) + 1, SYNF)):
        m = AttackModel(td={0: dict(flood_syn=1, syn_speed=7, syn_count=1 << 31, drop_pack=1)})
        m.ai[0]["synpps"] = pps
        assert run(m, [frame("syn")]) == [want]
    for flood_syn in (0, 1, 2):
        for cnt, want in ((5, FW), (6, SYNC)):
            m = AttackModel(td={0: dict(flood_syn=flood_syn, syn_speed=1000, syn_count=5, drop_pack=1)})
            m.ai[0]["syncount"] = cnt
            assert run(m, [frame("syn")]) == [want]
            assert m.info()["syncount_drop"] == int(want == SYNC) and m.ai[0]["syn_accum"] == 1
    m = AttackModel(td={0: dict(syn_count=5, drop_pack=0)})      # drop_pack gates the count branch too
    m.ai[0]["syncount"] = 6
    assert run(m, [frame("syn")]) == [FW]
    # the flood branches come first: held and over the count is 26
    m = AttackModel(td={0: dict(flood_syn=1, syn_speed=0, syn_count=0, drop_pack=1)})
    m.ai[0].update(synpps=1, syncount=1)
    assert run(m, [frame("syn")]) == [SYNF]


def test_hold_is_set_once_and_cleared_by_the_tick():
    """The first flood packet sets the hold with its launch's clock; a later clock does not move it; the tick clears at
    now == hold_time and not at hold_time - 1; a tick with nothing held clears nothing it should not."""
    m = AttackModel(td={0: dict(flood_udp=1, udp_speed=2, flood_syn=1, syn_speed=2, syn_count=99, drop_pack=1)},
                    hold_seconds=10)
    m.clock(NOW)
    assert run(m, [frame("udp")] * 3 + [frame("syn")] * 3) == [FW] * 6
    m.tick(NOW + 1)                                            # udppps = synpps = 3 > 2
    assert (m.ai[0]["udppps"], m.ai[0]["synpps"], m.ai[0]["syncount"]) == (3, 3, 3)
    assert run(m, [frame("udp"), frame("syn")]) == [UDPF, SYNF]
    assert (m.ai[0]["udp_flood_hold_time"], m.ai[0]["syn_flood_hold_time"]) == (NOW + 11, NOW + 11)
    m.clock(NOW + 5)
    assert run(m, [frame("udp"), frame("syn")]) == [UDPF, SYNF]
    assert (m.ai[0]["udp_flood_hold_time"], m.ai[0]["syn_flood_hold_time"]) == (NOW + 11, NOW + 11)
    m.tick(NOW + 10)                                           # pps 2 now, not above 2; hold_time - 1: still held
    assert m.ai[0]["udp_flood_hold"] == 1 and m.ai[0]["udppps"] == 2
    assert run(m, [frame("udp"), frame("syn")]) == [UDPF, SYNF]
    m.tick(NOW + 11)                                           # now == hold_time: cleared
    assert (m.ai[0]["udp_flood_hold"], m.ai[0]["udp_flood_hold_time"], m.ai[0]["syn_flood_hold"]) == (0, 0, 0)
    assert run(m, [frame("udp"), frame("syn")]) == [FW, FW]   # pps 1
    assert m.info()["udpflood_drop"] == 3 and m.info()["synflood_drop"] == 3


def test_land_only_on_tcp_syn():
    m = AttackModel({0: dict(land=1, drop_pack=1)})
    got = run(m, [frame("udp", A, A), frame("ack", A, A), frame("syn", A, A), frame("synack", A, A),
                  frame("syn", A, B), frame("rst", A, A)], syn_check=0)
    assert got == [FW, FW, LAND, LAND, FW, FW]
    assert m.ai[0]["syn_accum"] == 1 and m.info()["land_drop"] == 2     # land drops are not in syn_accum
    assert m.ai[0]["syncount_accum"] == 1 and m.ai[0]["udp_accum"] == 1
    e = run.last
    fl = (abi.F_TCP | abi.F_SYN)
    assert int(e["verdict"][2]) == LAND | (abi.ACT_DROP << 8) | (fl << 16)
    assert e["acl_hit"][2] == -1 and e["flow_hash"][2] == 0 and e["tuple"][2].tolist() == [A, A, 0, 6]
    assert e["flow_hash"][4] != 0 and e["tuple"][4][2] != 0
    # a SYN|ACK is a SYN for the flood monitor too, and is counted in syncount_accum when forwarded
    m = AttackModel()
    assert run(m, [frame("synack"), frame("ack")], syn_check=0) == [FW, FW]
    assert (m.ai[0]["syn_accum"], m.ai[0]["syncount_accum"]) == (1, 1)


def test_udp_monitor_sits_before_decode_udp():
    """l4len < 8 under a flood is 28, not 13; without a flood it stays 13 and is still counted; a length error too."""
    m = AttackModel(td={0: dict(flood_udp=1, udp_speed=0, drop_pack=1)})
    assert run(m, [frame("udp_short"), frame("udp_lenerr")]) == [ST["UDP_HEADER_ERR"], ST["UDP_LEN_ERR"]]
    assert m.ai[0]["udp_accum"] == 2
    m.tick(NOW)
    assert run(m, [frame("udp_short", vlan_tag=True), frame("udp_lenerr"), frame("udp")]) == [UDPF] * 3
    e = run.last
    assert int(e["verdict"][0]) == UDPF | (abi.ACT_DROP << 8) | (abi.F_VLAN << 16)
    assert e["tuple"][0].tolist() == [0x0A000001, 0x0A000002, 0, 17 | 0x100]
    c = e["counters"]
    assert (c["pkts"], c["l2_rx_ok"], c["vlan_rx_ok"], c["ipv4_rx_ok"], c["out_drop"]) == (3, 3, 1, 3, 3)
    assert sum(v for k, v in c.items() if k not in ("pkts", "l2_rx_ok", "vlan_rx_ok", "ipv4_rx_ok", "out_drop",
                                                     "rx_bytes")) == 0


def test_not_judged_not_counted():
    """A TCP SYN failing a length check, a TCP packet without SYN, fragments, other protocols: untouched, uncounted."""
    m = AttackModel({0: dict(land=1, drop_pack=1)},
                    {0: dict(flood_udp=1, flood_syn=1, udp_speed=0, syn_speed=0, syn_count=0, drop_pack=1)})
    m.ai[0].update(udppps=9, synpps=9, syncount=9)
    got = run(m, [frame("syn_lenerr", A, A), frame("syn_hdrerr", A, A), frame("ack"), frame("frag"), frame("icmp")])
    assert got == [ST["TCP_LEN_ERR"], ST["TCP_HEADER_ERR"], ST["FLOW_TCP_NO_SYN_FIRST"], ST["FRAG"],
                   ST["IPV4_UNSUPPORT"]]
    assert all(v == 0 for k, v in m.ai[0].items() if k.endswith("accum")) and m.ai[0]["syn_flood_hold"] == 0
    assert (run.last["verdict"] == run.ref["verdict"]).all()


def test_ports_are_independent_and_masked():
    m = AttackModel({1: dict(land=1, drop_pack=1)}, {2: dict(flood_udp=1, udp_speed=0, drop_pack=1)})
    m.ai[2]["udppps"] = 1
    m.ai[1]["udppps"] = 1
    fr = [frame("udp"), frame("udp"), frame("udp"), frame("syn", A, A), frame("syn", A, A), frame("udp")]
    assert run(m, fr, np.array([1, 2, 3, 1, 0, 6], np.uint8)) == [FW, UDPF, FW, LAND, FW, UDPF]   # 6 & 3 = 2
    assert [a["udp_accum"] for a in m.ai] == [0, 1, 2, 1] and [a["syn_accum"] for a in m.ai] == [1, 0, 0, 0]
    assert m.ai[2]["udp_flood_hold"] == 1 and m.ai[1]["udp_flood_hold"] == 0


def test_all_zero_rules_only_move_the_accumulators():
    m = AttackModel()
    fr = [frame(k, A, A if i & 1 else B, vlan_tag=bool(i & 2)) for i, k in enumerate(am.KINDS * 3)]
    run(m, fr, np.arange(len(fr), dtype=np.uint8) & 3)
    e, ref = run.last, run.ref
    for k in ("verdict", "flow_hash", "acl_hit", "tuple"):
        assert np.array_equal(e[k], ref[k]), k
    assert e["counters"] == dict(zip(abi.COUNTERS, (int(x) for x in ref["counters"])))
    assert sum(a["udp_accum"] for a in m.ai) == 9 and sum(a["syn_accum"] for a in m.ai) == 6
    assert sum(a["syncount_accum"] for a in m.ai) == 6 and not any(m.info()[k] for k in abi.ATTACK_TOTALS)


def test_composition_with_portscan_and_stream():
    """A monitor drop never reaches PortScan_Detect; syncount_accum excludes port-scan and ACL drops and includes what
    StreamTcp drops afterwards (a SYN|ACK is counted, then dropped as 22)."""
    m = AttackModel({0: dict(land=1, drop_pack=1)})
    ps = PortScanModel(exception_freq=0, capacity=8, cycles_per_second=1000)
    ps.clock(5000, NOW)
    fr = [frame("syn", A, A, dport=80), frame("syn", A, B, dport=81), frame("syn", A, A, dport=82),
          frame("syn", A, B, dport=83), frame("synack", B, A, dport=84)]
    got = run(m, fr, portscan=ps, now_seconds=NOW, stream=dict(track=1, midstream=0, async_oneside=0))
    assert got == [LAND, FW, LAND, ST["PORTSCAN_DROP"], ST["STREAM_MIDSTREAM_ONESIDE_OFF"]]
    assert ps.info()["ok"] == 2 and ps.info()["detected"] == 1 and len(ps.table) == 2
    assert m.ai[0]["syn_accum"] == 3 and m.ai[0]["syncount_accum"] == 2      # packets 1 and 4
    assert run.last["stream"]["syn_ack_count"] == 1


def test_frozen_scenario():
    """The model reproduces tests/golden/attack_v1.npz (gen_attack_golden.py's scripted intervals)."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_attack_golden as gen
    finally:
        sys.path.pop(0)
    g = np.load(GOLDEN / "attack_v1.npz")
    got = gen.run()
    assert sorted(got) == sorted(g.files)
    for k in g.files:
        assert got[k].dtype == g[k].dtype and np.array_equal(got[k], g[k]), k
    st = np.concatenate([g[f"verdict{b}"] & 0xFF for b in range(int(g["nbatch"][0]))])
    assert all((st == s).sum() > 5 for s in (LAND, SYNF, SYNC, UDPF))
    holds = np.array([g[f"state{b}"][:, [6, 8]].max() for b in range(int(g["nbatch"][0]))])
    assert holds.max() == 1 and holds[-1] == 0                  # held, then released


def _text(fn, *args):
    n = fn(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(*args, buf, n + 1) == n
    return buf.value.decode()


def _gen():
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_attack_golden as gen
    finally:
        sys.path.pop(0)
    return gen


def test_show_texts():
    """ppe_format_attack_stat and the attack section of ppe_format_pkt_stat_atk against the committed texts (and the
    generator still produces them); the older pkt_stat forms print what they printed."""
    lib, gen = abi.load(), _gen()
    info = gen.vec()
    want = (GOLDEN / "attack_stat_v1.txt").read_text()
    assert gen.attack_stat_text(info) == want
    assert _text(lib.ppe_format_attack_stat, C.byref(info)) == want
    assert want.count("interface") == 4 and "syn_count: -2147483647\n" in want and "udp_accum: 8589934636\n" in want
    small = C.create_string_buffer(16)
    assert lib.ppe_format_attack_stat(C.byref(info), small, 16) == len(want) and small.value.decode() == want[:15]
    assert lib.ppe_format_attack_stat(None, small, 16) == abi.PPE_EINVAL
    cnt = abi.Counters()
    for i in range(len(abi.COUNTERS)):
        cnt.c[i] = 1000 + 17 * i
    df = abi.DefragInfo()
    for k in range(9):
        df.st[k] = 501 + k
    df.teardrop, df.new_fcb, df.del_fcb = 510, 4242, 4141
    ps = abi.PortScanInfo()
    ps.drop = 987654321
    sec = (GOLDEN / "pkt_stat_atk_v1.txt").read_text()
    assert gen.attack_section_text(info, 510, 987654321) == sec
    v1, v2 = (GOLDEN / "pkt_stat_v1.txt").read_text(), (GOLDEN / "pkt_stat_v2.txt").read_text()
    got = _text(lib.ppe_format_pkt_stat_atk, C.byref(cnt), C.byref(df), 1, C.byref(ps), C.byref(info))
    cut = v2.index("attack stat:\n")
    assert got == v2[:cut] + sec and v2[cut:].count("\n") == sec.count("\n")
    assert _text(lib.ppe_format_pkt_stat_atk, C.byref(cnt), C.byref(df), 1, None, None) == v2
    assert _text(lib.ppe_format_pkt_stat_ps, C.byref(cnt), C.byref(df), 1, None) == v2
    assert _text(lib.ppe_format_pkt_stat_ex, C.byref(cnt), None, 0) == v1 == _text(lib.ppe_format_pkt_stat, C.byref(cnt))


def test_binding_matches_header():
    """Struct sizes, offsets and enum values of include/ppe_hip.h against ppe/abi.py (compiled with gcc)."""
    with tempfile.TemporaryDirectory() as td:
        src = Path(td) / "k.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppe_hip.h"\nint main(void){'
                       'printf("%d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                       "PPE_ST_ATTACK_LAND, PPE_ST_ATTACK_SYNFLOOD, PPE_ST_ATTACK_SYNCOUNT, PPE_ST_ATTACK_UDPFLOOD, "
                       "PPE_ST__ALL, PPE_ST__END, PPE_ST__COUNT, PPE_ABI_VERSION, sizeof(ppe_counters_t), "
                       "sizeof(ppe_attack_pd_t), sizeof(ppe_attack_td_t), sizeof(ppe_attack_cfg_t), "
                       "sizeof(ppe_attack_port_t), sizeof(ppe_attack_info_t), offsetof(ppe_attack_cfg_t, td), "
                       "offsetof(ppe_attack_cfg_t, hold_seconds), offsetof(ppe_attack_info_t, ai), "
                       "offsetof(ppe_attack_info_t, land_drop), offsetof(ppe_attack_port_t, syn_flood_hold));"
                       "return 0;}\n")
        exe = Path(td) / "k"
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       check=True)
        out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:9] == [25, 26, 27, 28, 29, 25, 24, 8, 256]
    assert out[:5] == [ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"], abi.ST_ALL]
    assert out[9:] == [C.sizeof(abi.AttackPd), C.sizeof(abi.AttackTd), C.sizeof(abi.AttackCfg), C.sizeof(abi.AttackPort),
                       C.sizeof(abi.AttackInfo), abi.AttackCfg.td.offset, abi.AttackCfg.hold_seconds.offset,
                       abi.AttackInfo.ai.offset, abi.AttackInfo.land_drop.offset, abi.AttackPort.syn_flood_hold.offset]
    assert [k for k, _ in abi.AttackPd._fields_] == list(am.PD_FIELDS)      # packet_detect's field order
    assert [k for k, _ in abi.AttackTd._fields_] == list(am.TD_FIELDS)      # traffic_detect's
    assert 2 * abi.ST_ALL <= 64 and abi.ST_ALL <= 32                        # the 2-bit action table, the 5-bit status
    assert all(abi.ST_NAME[s].startswith("ATTACK_") for s in range(25, 29))
    lib = abi.load()
    for name in ("ppe_attack_create", "ppe_attack_destroy", "ppe_attack_attach", "ppe_attack_set", "ppe_attack_clock",
                 "ppe_attack_tick", "ppe_attack_ports", "ppe_attack_info", "ppe_attack_clear_stat",
                 "ppe_format_attack_stat", "ppe_format_pkt_stat_atk", "ppe_pick_attack"):
        assert hasattr(lib, name) and name in abi.EXPORTS


def test_pick_attack_table():
    lib = abi.load()
    assert [lib.ppe_pick_attack(f, a) for f, a in ((0, 0), (0, 1), (1, 0), (1, 1))] == [0, 1, 0, 0]
    # independent of the port-scan choice: both may hold for one launch
    assert lib.ppe_pick_portscan(0, 1, 1) == 1 and lib.ppe_pick_attack(0, 1) == 1


def test_host_code_under_sanitizers():
    """tests/attack_san_main.c with csrc/ppe_stat.c and csrc/launch_plan.cpp under ASan + UBSan, as a program of its
    own: exact, tiny and zero capacities; its texts are the golden ones."""
    csrc = ROOT / "packet-process-engine_amd" / "csrc"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    inc = [f"-I{ROOT / 'include'}", f"-I{csrc}"]
    with tempfile.TemporaryDirectory() as td:
        t = Path(td)
        subprocess.run(["gcc", "-std=c11", "-D_GNU_SOURCE", *san, *inc, "-c", str(csrc / "ppe_stat.c"), "-o",
                        str(t / "stat.o")], check=True)
        subprocess.run(["gcc", "-std=c11", *san, *inc, "-c", str(ROOT / "tests" / "attack_san_main.c"), "-o",
                        str(t / "main.o")], check=True)
        subprocess.run(["g++", "-std=c++17", *san, *inc, "-c", str(csrc / "launch_plan.cpp"), "-o", str(t / "plan.o")],
                       check=True)
        subprocess.run(["g++", *san, str(t / "main.o"), str(t / "stat.o"), str(t / "plan.o"), "-o", str(t / "san")],
                       check=True)
        r = subprocess.run([str(t / "san")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    stat, pkt = r.stdout.split("\f")
    assert stat == (GOLDEN / "attack_stat_v1.txt").read_text()
    # (the program passes no reassembly table: its teardrop line prints 0)
    assert pkt.endswith((GOLDEN / "pkt_stat_atk_v1.txt").read_text().replace("teardrop: 510\n", "teardrop: 0\n"))
