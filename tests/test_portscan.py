"""The port-scan detector without a GPU: hand-derived known answers of the tests' serial model (tests/portscan_model.py,
PortScan_Detect / PortScan_timeout of dataplane/src/attack/dp_portscan.c), its frozen scenario
(tests/golden/portscan_v1.npz), the binding against the header, and the two new show-text functions.

The known answers use exception_freq = 3 and a rate of 1,000 cycles per second, so sequences stay short."""
import ctypes as C
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

import portscan_model as pm
from portscan_model import DETECTED, HOLD, NOMEM, OK, PortScanModel
from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
S = 0x0A000001   # the source
R = 1000         # oct_cpu_rate


def model(**kw):
    d = dict(exception_freq=3, hold_seconds=600, cycles_per_second=R)
    d.update(kw)
    return PortScanModel(**d)


def feed(m, now_cycles, now_seconds, ports, ts=None, sip=S):
    m.clock(now_cycles, now_seconds)
    return [m.detect(sip, p, now_seconds if ts is None else ts[i]) for i, p in enumerate(ports)]


def rec(m, sip=S):
    p = m.table[sip]
    return (p["last_dport"], p["exception"], p["last_exception"], p["last_cycle"], p["cycle"], p["hold"])


def test_first_create_and_counting_inside_a_window():
    m = model()
    assert feed(m, 5000, 100, [80]) == [OK]
    assert rec(m) == (80, 0, 0, 5000, 5000, 0)          # :155-160: port and last_cycle recorded, nothing counted
    assert feed(m, 5400, 100, [80, 81, 81, 82, 80]) == [OK] * 5
    assert rec(m) == (80, 3, 0, 5000, 5400, 0)          # three changes; last_cycle stays, cycle follows the clock
    assert m.info() == dict(new_pcb=1, del_pcb=0, ok=6, nomem=0, detected=0, hold=0, drop=0, live=1)


def test_roll_between_one_and_two_seconds():
    m = model()
    feed(m, 5000, 100, [80, 81, 82])
    assert feed(m, 6001, 101, [82]) == [OK]             # 1001 cycles: the roll, no port change
    assert rec(m) == (82, 0, 2, 6000, 6001, 0)          # last_cycle += rate, last_exception = exception, exception = 0
    assert feed(m, 6001, 101, [83]) == [OK]             # now 1 cycle into the window: `< rate`
    assert rec(m)[:3] == (83, 1, 2)


def test_exactly_rate_and_exactly_two_rate_reset():
    for dl in (R, 2 * R):
        m = model()
        feed(m, 5000, 100, [80, 81, 82, 83, 84])        # exception 4
        assert feed(m, 5000 + dl, 101, [85]) == [OK]    # neither `< rate` nor strictly between: the reset branch
        assert rec(m) == (85, 1, 0, 5000 + dl, 5000 + dl, 0), dl
    m = model()
    feed(m, 5000, 100, [80, 81, 82, 83, 84])
    assert feed(m, 5000 + 2 * R - 1, 101, [85]) == [DETECTED]   # strictly below 2 rate: the roll, 4 >= 3
    assert rec(m) == (85, 1, 4, 6000, 6999, 101 + 600)


def test_clock_behind_last_cycle_wraps_into_the_reset_branch():
    m = model()
    feed(m, 5000, 100, [80, 81])
    assert feed(m, 4000, 100, [82]) == [OK]             # now < last_cycle: the unsigned difference is huge
    assert rec(m) == (82, 1, 0, 4000, 4000, 0)


def test_detection_on_the_next_change_then_hold_then_release():
    m = model()
    feed(m, 5000, 100, [80, 81, 82, 83])                # exception 3
    assert feed(m, 6500, 101, [83]) == [OK]             # the roll without a change: last_exception 3, no detection
    assert rec(m)[:3] == (83, 0, 3)
    assert feed(m, 6600, 101, [83, 84, 85]) == [OK, DETECTED, HOLD]   # only a change detects (:166-174)
    assert rec(m) == (84, 1, 3, 6000, 6600, 701)        # hold = now_seconds + hold_seconds; cycle also for HOLD
    assert feed(m, 6700, 101, [1, 2], ts=[700, 700]) == [HOLD, HOLD]  # timestamp < hold
    assert rec(m)[:3] == (84, 1, 3) and rec(m)[4] == 6700
    # timestamp == hold: the hold clears and counting resumes (here in the `< rate` branch, last_exception still 3)
    assert feed(m, 6800, 101, [84, 86], ts=[701, 701]) == [OK, DETECTED]
    assert rec(m) == (86, 2, 3, 6000, 6800, 701)
    assert m.info() == dict(new_pcb=1, del_pcb=0, ok=7, nomem=0, detected=2, hold=3, drop=0, live=1)


def test_the_reset_branch_never_detects():
    m = model()
    feed(m, 5000, 100, [80, 81, 82, 83, 84])
    feed(m, 6500, 101, [84])                            # last_exception 4
    assert feed(m, 9000, 104, [85]) == [OK]             # > 2 s since last_cycle 6000: reset, no test
    assert rec(m) == (85, 1, 0, 9000, 9000, 0)


def test_hold_seconds_zero():
    m = model(hold_seconds=0)
    feed(m, 5000, 100, [80, 81, 82, 83])
    feed(m, 6500, 101, [83])
    # hold = now_seconds: the next packet's timestamp is not below it, so every change detects and none is held
    assert feed(m, 6600, 101, [84, 85, 85, 86]) == [DETECTED, DETECTED, OK, DETECTED]
    assert rec(m) == (86, 3, 3, 6000, 6600, 101)
    m = model(hold_seconds=0)
    feed(m, 5000, 0, [80, 81, 82, 83])
    feed(m, 6500, 0, [83])
    assert feed(m, 6600, 0, [84, 85]) == [DETECTED, DETECTED] and rec(m)[5] == 0   # hold 0 + 0: never set


def test_destination_port_zero():
    m = model()
    assert feed(m, 5000, 100, [0, 0, 80]) == [OK] * 3
    assert rec(m) == (80, 0, 0, 5000, 5000, 0)          # port 0 reads as "first create" again: nothing counted
    assert feed(m, 5500, 100, [0]) == [OK]              # 80 -> 0 is a change
    assert rec(m) == (0, 1, 0, 5000, 5500, 0)
    assert feed(m, 5600, 100, [443]) == [OK]            # last_dport 0: first create, re-arms last_cycle, no count
    assert rec(m) == (443, 1, 0, 5600, 5600, 0)


def test_aging_boundaries():
    m = model()
    feed(m, 5000, 100, [80])
    feed(m, 5000, 100, [80], sip=S + 1)
    feed(m, 5001, 100, [80], sip=S + 2)
    assert m.timeout(5000 + 20 * R) == 0                # == 20 rate stays
    assert m.timeout(4000) == 0                         # now <= cycle stays
    assert m.timeout(5001 + 20 * R) == 2                # > 20 rate for the two records stamped 5000
    assert set(m.table) == {S + 2} and m.info()["del_pcb"] == 2


def test_capacity_nomem_in_first_appearance_order():
    m = model(capacity=2)
    m.clock(5000, 100)
    got = [m.detect(S + k, 80, 100) for k in (0, 1, 2, 0, 2, 3, 1)]
    assert got == [OK, OK, NOMEM, OK, NOMEM, NOMEM, OK]
    assert set(m.table) == {S, S + 1} and m.info()["nomem"] == 3 and m.info()["new_pcb"] == 2
    assert m.timeout(5000 + 21 * R) == 2                # nothing frees within a batch; aging does
    assert m.detect(S + 3, 80, 100) == OK


def test_disabled_and_forward_action():
    m = model(able=0)
    assert m.detect(S, 80, 0) is None and not m.table
    ref = dict(verdict=np.array([abi.ST["ACL_FW"] | ((abi.F_L4 | abi.F_ACL) << 16)] * 6, np.uint32),
               flow_hash=np.arange(6, dtype=np.uint32), acl_hit=np.arange(6, dtype=np.int32),
               tuple=np.array([[S, 9, 7 | (p << 16), 17] for p in (80, 81, 82, 83, 84, 85)], np.uint32),
               counters=np.zeros(32, np.uint64))
    c = {k: i for i, k in enumerate(abi.COUNTERS)}
    for k in ("acl_fw", "flow_proc_ok", "out_fw", "pkts"):
        ref["counters"][c[k]] = 6
    for action in (0, 1):
        m = model(action=action, exception_freq=0)       # freq 0: the first change detects
        m.clock(5000, 100)
        e = m.expected(ref, None, now_seconds=100)
        assert e["results"].tolist() == [OK, DETECTED, HOLD, HOLD, HOLD, HOLD]
        if action:                                       # forwarded unchanged; detection and state still ran
            assert (e["verdict"] == ref["verdict"]).all() and (e["acl_hit"] == ref["acl_hit"]).all()
            assert e["counters"]["acl_fw"] == 6 and m.info()["drop"] == 0
        else:
            assert (e["verdict"][1:] == (abi.ST["PORTSCAN_DROP"] | (abi.ACT_DROP << 8) | (abi.F_L4 << 16))).all()
            assert e["acl_hit"].tolist() == [0, -1, -1, -1, -1, -1] and (e["flow_hash"] == ref["flow_hash"]).all()
            cn = e["counters"]
            assert (cn["acl_fw"], cn["flow_proc_ok"], cn["out_fw"], cn["flow_proc_fail"], cn["out_drop"], cn["pkts"],
                    cn["acl_drop"]) == (1, 1, 1, 5, 5, 6, 0)
            assert m.info()["drop"] == 5


def test_frozen_scenario():
    """The model reproduces tests/golden/portscan_v1.npz (gen_portscan_golden.py's scripted batches)."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_portscan_golden as gen
    finally:
        sys.path.pop(0)
    g = np.load(GOLDEN / "portscan_v1.npz")
    got = gen.run()
    assert sorted(got) == sorted(g.files)
    for k in g.files:
        assert got[k].dtype == g[k].dtype and np.array_equal(got[k], g[k]), k
    assert sum(int((g[f"res{b}"] == DETECTED).sum()) for b in range(8)) > 0
    assert sum(int((g[f"res{b}"] == HOLD).sum()) for b in range(8)) > 0
    assert sum(int((g[f"res{b}"] == NOMEM).sum()) for b in range(8)) > 0 and int(g["freed5"][0]) == 6


def test_binding_matches_header():
    """Struct sizes and enum values of include/ppe_hip.h against ppe/abi.py (compiled with gcc)."""
    with tempfile.TemporaryDirectory() as td:
        src = Path(td) / "k.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppe_hip.h"\nint main(void){'
                       'printf("%d %d %zu %zu %zu %zu %zu %zu %d\\n", PPE_ST_PORTSCAN_DROP, PPE_ST__END, '
                       "sizeof(ppe_portscan_cfg_t), sizeof(ppe_portscan_info_t), sizeof(ppe_portscan_entry_t), "
                       "offsetof(ppe_portscan_cfg_t, cycles_per_second), offsetof(ppe_portscan_info_t, cfg), "
                       "offsetof(ppe_portscan_entry_t, last_cycle), PPE_ABI_VERSION);return 0;}\n")
        exe = Path(td) / "k"
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       check=True)
        out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [abi.ST["PORTSCAN_DROP"], abi.ST_END, C.sizeof(abi.PortScanCfg), C.sizeof(abi.PortScanInfo),
                   abi.PORTSCAN_ENTRY_DTYPE.itemsize, abi.PortScanCfg.cycles_per_second.offset,
                   abi.PortScanInfo.cfg.offset, abi.PORTSCAN_ENTRY_DTYPE.fields["last_cycle"][1], abi.ABI_VERSION]
    assert out[:3] == [24, 25, 40] and abi.ST_NAME[24] == "PORTSCAN_DROP"
    assert abi.ST_COUNT == 24 and 2 * abi.ST_END <= 64                      # the kernels' 2-bit action table
    lib = abi.load()
    for name in ("ppe_portscan_create", "ppe_portscan_destroy", "ppe_portscan_attach", "ppe_portscan_clock",
                 "ppe_portscan_set", "ppe_portscan_age", "ppe_portscan_info", "ppe_portscan_dump",
                 "ppe_format_pkt_stat_ps", "ppe_format_fw_config"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert [lib.ppe_pick_portscan(f, a, able) for f, a, able in ((0, 1, 1), (1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 1, 2))] \
        == [1, 0, 0, 0, 0]


def _text(fn, *args):
    n = fn(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(*args, buf, n + 1) == n
    return buf.value.decode()


def test_fw_config_text():
    """The four port-scan lines of dp_cmd.c:2578-2590, built here from its format strings."""
    lib = abi.load()

    def want(able, action, hold, freq):
        return ("portscan attack detect stat: %s\n" % ("enable" if able else "disable") +
                "portscan attack detect action: %s\n" % ("fw" if action else "drop") +
                "flood hold time: %d\n" % hold + "portscan_exception_freq: %d\n" % freq)
    assert _text(lib.ppe_format_fw_config, None) == want(1, 0, 600, 50)   # the reference's defaults
    for able, action, hold, freq in ((0, 1, 30, 7), (1, 1, 0, 0), (1, 0, 86400, 65535)):
        cfg = abi.PortScanCfg(able, action, freq, hold, 0, 0, 0, 0)
        assert _text(lib.ppe_format_fw_config, C.byref(cfg)) == want(able, action, hold, freq)
    small = C.create_string_buffer(20)                   # snprintf semantics
    assert lib.ppe_format_fw_config(None, small, 20) == len(want(1, 0, 600, 50)) and len(small.value) == 19


def test_pkt_stat_text_with_portscan_drop():
    """ppe_format_pkt_stat_ps = ppe_format_pkt_stat_ex with the portscan_drop line from the table's info; the
    existing forms print what they printed (the golden texts of tests/test_stat_format.py)."""
    lib = abi.load()
    cnt = abi.Counters()
    for i in range(len(abi.COUNTERS)):
        cnt.c[i] = 1000 + 17 * i
    df = abi.DefragInfo()
    for k in range(9):
        df.st[k] = 501 + k
    df.teardrop, df.new_fcb, df.del_fcb = 510, 4242, 4141
    v1, v2 = (GOLDEN / "pkt_stat_v1.txt").read_text(), (GOLDEN / "pkt_stat_v2.txt").read_text()
    assert "portscan_drop: 0\n" in v1 and v1.count("portscan_drop") == 1
    assert _text(lib.ppe_format_pkt_stat_ex, C.byref(cnt), C.byref(df), 1) == v2          # unchanged
    assert _text(lib.ppe_format_pkt_stat_ex, C.byref(cnt), None, 0) == v1
    assert _text(lib.ppe_format_pkt_stat, C.byref(cnt)) == v1
    info = abi.PortScanInfo()
    info.drop = 987654321
    assert _text(lib.ppe_format_pkt_stat_ps, C.byref(cnt), C.byref(df), 1, C.byref(info)) == \
        v2.replace("portscan_drop: 0\n", "portscan_drop: %ld\n" % 987654321)
    assert _text(lib.ppe_format_pkt_stat_ps, C.byref(cnt), None, 0, C.byref(info)) == \
        v1.replace("portscan_drop: 0\n", "portscan_drop: 987654321\n")
    assert _text(lib.ppe_format_pkt_stat_ps, C.byref(cnt), C.byref(df), 1, None) == v2


assert pm.RESULTS == ("ok", "nomem", "detected", "hold")
