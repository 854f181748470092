"""The host side of the one-launch flow kernel and of the flow table behind Decode, without a GPU: the planner that picks
the one-launch kernel (csrc/launch_plan.cpp) and its cutoff, the new symbols and their prototypes, include/ppe_decode.h's
globals at their start values, and Decode with the flow table on and no device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent


def cutoff():
    text = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()
    return int(re.search(r"#define PPE_FLOW_SMALL_CUTOFF (\d+)u", text).group(1))


def test_planner_picks_the_one_launch_kernel_up_to_the_cutoff():
    lib = abi.load()
    pick, c = lib.ppe_pick_flow_small, cutoff()
    assert [pick(n, 1, 0) for n in (1, 2, 64, c - 1, c)] == [1] * 5
    assert [pick(n, 1, 0) for n in (c + 1, 8000, 1 << 20)] == [0, 0, 0]   # (the fail-fast test's 8,000: two launches)
    assert pick(0, 1, 0) == 0
    assert [pick(n, 0, 0) for n in (1, 64, c, c + 1)] == [0] * 4          # PPE_FLOW_SMALL=0, or the failure hook armed
    assert [pick(n, 1, 1) for n in (1, 64, c, c + 1)] == [0] * 4          # monitors flow-attached


def test_cutoff_conditions():
    c = cutoff()
    assert c % 64 == 0 and 64 <= c <= 2048


def test_new_symbols_resolve():
    lib = abi.load()
    for name in ("ppe_classify_flow_host", "ppe_flow_launch_info", "ppe_pick_flow_small", "DP_Flow_Clock",
                 "DP_Flow_Age"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert C.c_uint32.in_dll(lib, "flow_able").value == 0
    assert C.c_uint32.in_dll(lib, "flow_item_num").value == 100000
    assert lib.ppe_abi_version() == 8
    assert lib.ppe_classify_flow_host(None, None, None, None, 0) == abi.PPE_EINVAL
    assert lib.ppe_flow_launch_info(None, None, None) == abi.PPE_EINVAL
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    assert "int  ppe_classify_flow_host(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out," in hdr
    assert "int  ppe_flow_launch_info(ppe_ctx_t *ctx, uint32_t *kind, uint32_t *launches);" in hdr
    internal = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()
    assert "uint32_t ppe_pick_flow_small(uint32_t n, int small_allowed, int atk_flow_attached);" in internal
    dec = (ROOT / "include" / "ppe_decode.h").read_text()
    for proto in ("extern uint32_t flow_able;", "extern uint32_t flow_item_num;",
                  "void DP_Flow_Clock(uint64_t now_seconds);",
                  "int  DP_Flow_Age(uint64_t now_seconds, uint64_t *deleted);"):
        assert proto in dec


def test_decode_header_globals_and_start_values(tmp_path):
    """include/ppe_decode.h alone compiles with gcc, names the two globals and the two entry points, and a program
    linked against the library reads the start values: the flow table off, a pool of 100,000; aging without a table
    is PPE_OK with nothing deleted."""
    src = tmp_path / "fl.c"
    src.write_text('#include <stdio.h>\n#include "ppe_decode.h"\n'
                   "int main(void) {\n"
                   "    void (*clk)(uint64_t) = DP_Flow_Clock;\n"
                   "    int (*age)(uint64_t, uint64_t *) = DP_Flow_Age;\n"
                   "    uint64_t deleted = 7;\n"
                   "    clk(5);\n"
                   "    const int rc = age(1000, &deleted);\n"
                   '    printf("%u %u %d %llu %d\\n", flow_able, flow_item_num, rc, (unsigned long long)deleted,\n'
                   "           age(1000, 0));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "fl"
    lib = ROOT / "packet-process-engine_amd"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), f"-L{lib}", "-lppe_hip",
                    f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["0", "100000", "0", "0", "0"]


def test_decode_without_a_device_drops_everything_with_the_flow_table_on():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-only bookkeeping test (a GPU would classify the bursts)")
    HOOK = C.CFUNCTYPE(None, C.POINTER(abi.Mbuf))
    lib = abi.load()
    lib.DP_Acl_Rule_Release()  # no context: flushes fail with PPE_ENODEV
    lib.ppe_set_output_hooks.argtypes = [HOOK, HOOK, HOOK]
    got = {}

    def mk(key):
        return HOOK(lambda m: got.setdefault(key, []).append(C.addressof(m.contents)))
    hooks = (mk("fw"), mk("drop"), mk("punt"))
    able = C.c_uint32.in_dll(lib, "flow_able")
    lib.ppe_set_output_hooks(*hooks)
    able.value = 1
    try:
        mb = (abi.Mbuf * 7)()
        lib.Decode_Set_Burst(4)
        lib.DP_Flow_Clock(1000)
        for i in range(7):
            lib.Decode(C.byref(mb[i]))
        assert len(got["drop"]) == 4
        assert lib.Decode_Flush() == -19  # PPE_ENODEV
        base = C.addressof(mb)
        assert sorted((a - base) // C.sizeof(abi.Mbuf) for a in got["drop"]) == list(range(7))
        assert "fw" not in got and "punt" not in got
        deleted = C.c_uint64(3)
        assert lib.DP_Flow_Age(2000, C.byref(deleted)) == 0 and deleted.value == 0
    finally:
        able.value = 0
        lib.ppe_set_output_hooks(HOOK(), HOOK(), HOOK())
        lib.Decode_Set_Burst(4096)
