"""The attack monitors with TCP sessions on the flow path without a device: the planner
(ppe_pick_flow_stream_monitors, csrc/launch_plan.cpp) over every input on both sides of the maximum, its equality with
ppe_pick_flow_stream wherever the switch is off, and the additive ABI (the new names, the version and
ppe_flow_stream_entry_t unchanged)."""
import ctypes as C
import itertools
import re
from pathlib import Path

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
INTERNAL = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()
MAX = int(re.search(r"#define PPE_FLOW_ST_MAX (\d+)u", INTERNAL).group(1))
PLAIN, KERNEL, REFUSE, KERNEL_ATK = 0, 1, 2, 3
SIZES = (1, 2, 63, 64, 65, MAX - 1, MAX, MAX + 1, 2 * MAX, 1 << 20)


def every_input():
    """(n, attached, track, midstream, async_oneside, reasm, ps, atk): every flag 0 / 1 (track also 2: not 1 is off)."""
    for n in SIZES:
        for f in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
            yield (n,) + f


def test_switch_off_is_ppe_pick_flow_stream():
    lib = abi.load()
    for a in every_input():
        for on in (0, 2, 7):  # (only 1 is on; the context refuses the other values before they get here)
            assert lib.ppe_pick_flow_stream_monitors(*a, on) == lib.ppe_pick_flow_stream(*a), (a, on)


def test_switch_on_over_every_input():
    """The answer written out from the interface's rules, not from ppe_pick_flow_stream."""
    lib = abi.load()
    seen = set()
    for a in every_input():
        n, attached, track, mid, asy, reasm, ps, atk = a
        if not attached or track != 1:
            want = PLAIN                      # the switch changes nothing without sessions that run
        elif mid or asy or reasm:
            want = REFUSE
        elif ps:
            want = REFUSE                     # a port-scan table flow-attached as well, whatever its able
        elif n > MAX:
            want = REFUSE
        else:
            want = KERNEL_ATK if atk else KERNEL
        assert lib.ppe_pick_flow_stream_monitors(*a, 1) == want, a
        seen.add(want)
    assert seen == {PLAIN, KERNEL, REFUSE, KERNEL_ATK}
    assert lib.ppe_pick_flow_stream_monitors(MAX, 1, 1, 0, 0, 0, 0, 1, 1) == KERNEL_ATK
    assert lib.ppe_pick_flow_stream_monitors(MAX + 1, 1, 1, 0, 0, 0, 0, 1, 1) == REFUSE
    # ppe_pick_flow_stream itself keeps refusing the monitors
    assert lib.ppe_pick_flow_stream(1, 1, 1, 0, 0, 0, 0, 1) == REFUSE


def test_additive_abi():
    lib = abi.load()
    assert lib.ppe_abi_version() == 8
    for name in ("ppe_flow_stream_monitors", "ppe_pick_flow_stream_monitors"):
        assert hasattr(lib, name) and name in abi.EXPORTS, name
    assert C.sizeof(abi.FlowStreamEntry) == 68 and abi.FlowStreamEntry.pad.offset == 19
    assert int(re.search(r"#define PPE_FST_KERNEL_ATK (\d+)u", INTERNAL).group(1)) == KERNEL_ATK
    assert lib.ppe_flow_stream_monitors(None, 1) == abi.PPE_EINVAL
