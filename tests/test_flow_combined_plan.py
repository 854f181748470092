"""The host side of ppe_flow_combine, without a GPU: the planner's full truth table (csrc/launch_plan.cpp,
ppe_pick_flow_combined), the new symbols and their prototypes through the library, the ABI version."""
import itertools
from pathlib import Path

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
INTERNAL = ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h"
PLAIN, KERNEL, REFUSE = 0, 1, 2      # ppe_pick_flow_portscan's answers
NONE, COMBINED, REFUSED = 0, 1, 2    # ppe_pick_flow_combined's


def test_planner_truth_table():
    """0: not the combination (fps PLAIN, or no monitors flow-attached); 1: fps KERNEL, monitors, combine on; 2: monitors
    flow-attached and fps != PLAIN with combine off or fps REFUSE."""
    pick = abi.load().ppe_pick_flow_combined
    for fps, atk, on in itertools.product((PLAIN, KERNEL, REFUSE), (0, 1), (0, 1)):
        want = NONE if fps == PLAIN or not atk else COMBINED if fps == KERNEL and on else REFUSED
        assert pick(fps, atk, on) == want, (fps, atk, on)
    # written out, the twelve rows
    assert [pick(PLAIN, a, o) for a in (0, 1) for o in (0, 1)] == [NONE] * 4
    assert [pick(KERNEL, a, o) for a in (0, 1) for o in (0, 1)] == [NONE, NONE, REFUSED, COMBINED]
    assert [pick(REFUSE, a, o) for a in (0, 1) for o in (0, 1)] == [NONE, NONE, REFUSED, REFUSED]
    assert pick(KERNEL, 1, 2) == REFUSED      # (the switch only holds 0 or 1; anything else is not "on")


def test_the_two_planners_composed_over_sizes():
    lib = abi.load()
    m = lib.ppe_flow_portscan_max()

    def plan(n, table, able, atk, on):
        return lib.ppe_pick_flow_combined(lib.ppe_pick_flow_portscan(n, table, able), atk, on)
    assert [plan(n, 1, 1, 1, 1) for n in (1, 63, 64, 65, m - 1, m)] == [COMBINED] * 6
    assert [plan(n, 1, 1, 1, 1) for n in (m + 1, 8000)] == [REFUSED] * 2
    assert [plan(n, 1, 1, 1, 0) for n in (1, m, m + 1)] == [REFUSED] * 3
    # only one of the two attached, or able 0: never the combination, whatever the switch
    for n, on in itertools.product((1, 64, m, m + 1, 8000), (0, 1)):
        assert plan(n, 1, 1, 0, on) == NONE and plan(n, 0, 1, 1, on) == NONE and plan(n, 1, 0, 1, on) == NONE


def test_new_symbols_and_prototypes():
    lib = abi.load()
    for name in ("ppe_flow_combine", "ppe_pick_flow_combined"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert lib.ppe_abi_version() == 8
    assert lib.ppe_flow_combine(None, 1) == abi.PPE_EINVAL
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    assert "int  ppe_flow_combine(ppe_ctx_t *ctx, uint32_t on);" in hdr
    assert "#define PPE_ABI_VERSION 8" in hdr
    text = INTERNAL.read_text()
    assert "uint32_t ppe_pick_flow_combined(uint32_t fps, int atk_flow_attached, uint32_t combine_on);" in text
    assert "int ppe_launch_flow_portscan_attack(" in text
    from ppe import Engine
    assert callable(Engine.flow_combine)
