"""The host side of the port-scan detector on the flow-table path, without a GPU: the planner that picks plain kernels,
the kernel with the detector inside, or a refusal (csrc/launch_plan.cpp) on both sides of PPE_FLOW_PS_MAX, the new
symbols and their prototypes, include/ppe_decode.h's new global at its start value, and Decode with it on and no
device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
INTERNAL = ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h"
PLAIN, KERNEL, REFUSE = 0, 1, 2


def ps_max():
    return int(re.search(r"#define PPE_FLOW_PS_MAX (\d+)u", INTERNAL.read_text()).group(1))


def test_planner_on_both_sides_of_the_maximum():
    lib = abi.load()
    pick, m = lib.ppe_pick_flow_portscan, ps_max()
    assert m in (512, 1024, 2048) and lib.ppe_flow_portscan_max() == m
    assert [pick(n, 1, 1) for n in (1, 63, 64, 65, m - 1, m)] == [KERNEL] * 6
    assert [pick(n, 1, 1) for n in (m + 1, 8000, 1 << 20)] == [REFUSE] * 3
    # nothing flow-attached, or portscan_able off (dp_portscan.c:238: any value but 1): today's kernels at every size
    for n in (1, 64, m, m + 1, 8000, 1 << 20):
        assert pick(n, 0, 1) == PLAIN and pick(n, 1, 0) == PLAIN and pick(n, 0, 0) == PLAIN and pick(n, 1, 2) == PLAIN


def test_new_symbols_and_prototypes():
    lib = abi.load()
    for name in ("ppe_flow_portscan_attach", "ppe_flow_portscan_max", "ppe_flow_portscan_rounds",
                 "ppe_pick_flow_portscan"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert lib.ppe_abi_version() == 8
    assert lib.ppe_flow_portscan_attach(None, None) == abi.PPE_EINVAL
    assert lib.ppe_flow_portscan_rounds(None, None) == abi.PPE_EINVAL
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    assert "int  ppe_flow_portscan_attach(ppe_ctx_t *ctx, ppe_portscan_t *ps);" in hdr
    assert "uint32_t ppe_flow_portscan_max(void);" in hdr
    assert "int  ppe_flow_portscan_rounds(ppe_ctx_t *ctx, uint32_t *rounds);" in hdr
    text = INTERNAL.read_text()
    assert "uint32_t ppe_pick_flow_portscan(uint32_t n, int flow_attached, uint32_t able);" in text
    assert "extern uint32_t flow_portscan_able;" in (ROOT / "include" / "ppe_decode.h").read_text()
    assert C.c_uint32.in_dll(lib, "flow_portscan_able").value == 0


def test_decode_header_global_and_start_value(tmp_path):
    """include/ppe_decode.h alone compiles with gcc and names the new global; a program linked against the library reads
    its start value beside the other switches': everything off."""
    src = tmp_path / "fps.c"
    src.write_text('#include <stdio.h>\n#include "ppe_decode.h"\n'
                   "int main(void) {\n"
                   '    printf("%u %u %u\\n", flow_portscan_able, flow_able, portscan_able);\n'
                   "    flow_portscan_able = 1;\n"
                   '    printf("%u %p\\n", flow_portscan_able, (void *)DP_PortScan_Table());\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "fps"
    lib = ROOT / "packet-process-engine_amd"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), f"-L{lib}", "-lppe_hip",
                    f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[:4] == ["0", "0", "0", "1"] and out[4] in ("(nil)", "0x0")  # no table before a flush needs one


def test_decode_without_a_device_drops_everything_with_the_detector_on():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-only bookkeeping test (a GPU would classify the bursts)")
    HOOK = C.CFUNCTYPE(None, C.POINTER(abi.Mbuf))
    lib = abi.load()
    lib.DP_Acl_Rule_Release()  # no context: flushes fail with PPE_ENODEV
    lib.ppe_set_output_hooks.argtypes = [HOOK, HOOK, HOOK]
    lib.DP_PortScan_Table.restype = C.c_void_p
    got = {}

    def mk(key):
        return HOOK(lambda m: got.setdefault(key, []).append(C.addressof(m.contents)))
    hooks = (mk("fw"), mk("drop"), mk("punt"))
    flow, fps = C.c_uint32.in_dll(lib, "flow_able"), C.c_uint32.in_dll(lib, "flow_portscan_able")
    lib.ppe_set_output_hooks(*hooks)
    try:
        mb = (abi.Mbuf * 6)()
        lib.Decode_Set_Burst(3)
        for on in (0, 1):  # without flow_able the new global has no effect; with it, the burst still ends in the drop hook
            flow.value, fps.value = on, 1
            got.clear()
            lib.DP_PortScan_Clock(10**9, 1000)
            for i in range(5):
                lib.Decode(C.byref(mb[i]))
            assert len(got["drop"]) == 3
            assert lib.Decode_Flush() == -19  # PPE_ENODEV
            base = C.addressof(mb)
            assert sorted((a - base) // C.sizeof(abi.Mbuf) for a in got["drop"]) == list(range(5))
            assert "fw" not in got and "punt" not in got
            assert lib.DP_PortScan_Table() is None  # nothing was created
            freed = C.c_uint64(3)
            assert lib.DP_PortScan_Age(10**12, C.byref(freed)) == 0 and freed.value == 0
    finally:
        flow.value = fps.value = 0
        lib.ppe_set_output_hooks(HOOK(), HOOK(), HOOK())
        lib.Decode_Set_Burst(4096)
