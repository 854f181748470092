"""The port-scan detector with TCP sessions on the flow path without a device: the planner
(ppe_pick_flow_stream_portscan, csrc/launch_plan.cpp) over its whole truth table on both sides of the maximum, its
equality with ppe_pick_flow_stream_monitors wherever the switch is off or no table is flow-attached, and the additive
ABI (the new names and prototypes; the version and ppe_flow_stream_entry_t unchanged)."""
import ctypes as C
import itertools
import re
from pathlib import Path

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
INTERNAL = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()
HEADER = (ROOT / "include" / "ppe_hip.h").read_text()
ST_MAX = int(re.search(r"#define PPE_FLOW_ST_MAX (\d+)u", INTERNAL).group(1))
PS_MAX = int(re.search(r"#define PPE_FLOW_PS_MAX (\d+)u", INTERNAL).group(1))
MAX = min(ST_MAX, PS_MAX)
PLAIN, KERNEL, REFUSE, KERNEL_ATK, KERNEL_PS, KERNEL_PS_ATK = 0, 1, 2, 3, 4, 5
SIZES = (1, 63, 64, 65, MAX - 1, MAX, MAX + 1, 2 * MAX, 1 << 20)


def every_input():
    """(n, attached, track, midstream, async_oneside, reasm, ps, atk, monitors_on, able, combine_on): every flag 0 / 1
    (track and able also 2: not 1 is off)."""
    for n in SIZES:
        for f in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)):
            yield (n,) + f


def call(lib, a, on):
    n, attached, track, mid, asy, reasm, ps, atk, mon, able, comb = a
    return lib.ppe_pick_flow_stream_portscan(n, attached, track, mid, asy, reasm, ps, atk, mon, able, on, comb)


def test_switch_off_or_no_table_is_ppe_pick_flow_stream_monitors():
    lib = abi.load()
    for a in every_input():
        base = lib.ppe_pick_flow_stream_monitors(*a[:9])
        for on in (0, 2, 7):  # (only 1 is on; the context refuses the other values before they get here)
            assert call(lib, a, on) == base, (a, on)
        if not a[6]:
            assert call(lib, a, 1) == base, a


def test_switch_on_over_every_input():
    """The answer written out from the interface's rules, not from the other planners."""
    lib = abi.load()
    seen = set()
    for a in every_input():
        n, attached, track, mid, asy, reasm, ps, atk, mon, able, comb = a
        detector = ps and able == 1
        if not attached or track != 1:
            want = PLAIN                      # the switch changes nothing without sessions that run
        elif mid or asy or reasm:
            want = REFUSE
        elif n > MAX:
            want = REFUSE
        elif not detector:                    # no table, or its detector off: kinds 5 / 6 and their refusal
            want = (KERNEL_ATK if mon == 1 else REFUSE) if atk else KERNEL
        elif not atk:
            want = KERNEL_PS
        else:                                 # both pairs must have been opted into
            want = KERNEL_PS_ATK if (mon == 1 and comb == 1) else REFUSE
        assert call(lib, a, 1) == want, a
        seen.add(want)
    assert seen == {PLAIN, KERNEL, REFUSE, KERNEL_ATK, KERNEL_PS, KERNEL_PS_ATK}
    f = lib.ppe_pick_flow_stream_portscan
    assert f(MAX, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0) == KERNEL_PS and f(MAX + 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0) == REFUSE
    assert f(MAX, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1) == KERNEL_PS_ATK and f(MAX + 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1) == REFUSE
    assert f(1, 1, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1) == REFUSE and f(1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0) == REFUSE
    # the older planners keep refusing a table flow-attached, whatever its able
    assert lib.ppe_pick_flow_stream_monitors(1, 1, 1, 0, 0, 0, 1, 0, 1) == REFUSE
    assert lib.ppe_pick_flow_stream(1, 1, 1, 0, 0, 0, 1, 0) == REFUSE


def test_additive_abi():
    lib = abi.load()
    assert lib.ppe_abi_version() == 8
    for name in ("ppe_flow_stream_portscan", "ppe_pick_flow_stream_portscan"):
        assert hasattr(lib, name) and name in abi.EXPORTS, name
    assert re.search(r"int\s+ppe_flow_stream_portscan\(ppe_ctx_t \*ctx, uint32_t on\);", HEADER)
    proto = re.search(r"uint32_t ppe_pick_flow_stream_portscan\(([^)]*)\);", INTERNAL).group(1)
    assert [p.split()[-1] for p in proto.split(",")] == ["n", "attached", "track", "midstream", "async_oneside", "reasm",
                                                         "ps_flow_attached", "atk_flow_attached", "monitors_on", "able",
                                                         "portscan_on", "combine_on"]
    assert C.sizeof(abi.FlowStreamEntry) == 68 and abi.FlowStreamEntry.pad.offset == 19
    assert int(re.search(r"#define PPE_FST_KERNEL_PS (\d+)u", INTERNAL).group(1)) == KERNEL_PS
    assert int(re.search(r"#define PPE_FST_KERNEL_PS_ATK (\d+)u", INTERNAL).group(1)) == KERNEL_PS_ATK
    assert lib.ppe_flow_stream_portscan(None, 1) == abi.PPE_EINVAL
    for sym in ("ppe_launch_flow_stream_portscan", "ppe_launch_flow_stream_portscan_attack"):
        assert hasattr(lib, sym), sym
