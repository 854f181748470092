"""The host side of ppe_classify_flow_host_ports and of the monitors behind Decode, without a GPU: the planner that picks
the one-launch kernel with the monitors in it (csrc/launch_plan.cpp, ppe_pick_flow_small_attack) on both sides of the
cutoff and under each of its three flags, the older planners unchanged, the new symbols with their prototypes, the new
unit in the build, the start values through a linked C program that includes ppe_decode.h alone, and Decode without a
device."""
import ctypes as C
import itertools
import re
import subprocess
from pathlib import Path

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "packet-process-engine_amd"
INTERNAL = (PKG / "csrc" / "ppe_internal.h").read_text()
CUTOFF = int(re.search(r"#define PPE_FLOW_SMALL_CUTOFF (\d+)u", INTERNAL).group(1))
# the planner's own bound for the kernel with the monitors in it: at most CUTOFF, lowered to what
# tools/ab_flow_host_ports.py's measurement supports
ACUT = int(re.search(r"#define PPE_FLOW_SMALL_ATK_CUTOFF (\d+)u", INTERNAL).group(1))
SIZES = (0, 1, 63, 64, 65, ACUT - 1, ACUT, ACUT + 1, CUTOFF - 1, CUTOFF, CUTOFF + 1, 4133, 1 << 20)


def test_planner_truth_table():
    """1 exactly when 1 <= n <= the cutoff, the table allows it, monitors are flow-attached and the batch is a chunk of
    the ports call."""
    assert 64 <= ACUT <= CUTOFF and ACUT % 64 == 0
    pick = abi.load().ppe_pick_flow_small_attack
    for n, allowed, atk, ports in itertools.product(SIZES, (0, 1), (0, 1), (0, 1)):
        want = 1 if (1 <= n <= ACUT and allowed and atk and ports) else 0
        assert pick(n, allowed, atk, ports) == want, (n, allowed, atk, ports)
    # written out: each flag alone turns it off on both sides of the cutoff
    assert [pick(n, 1, 1, 1) for n in (1, ACUT, ACUT + 1, CUTOFF + 1)] == [1, 1, 0, 0]
    assert [pick(n, 0, 1, 1) for n in (1, ACUT, ACUT + 1, CUTOFF + 1)] == [0] * 4  # PPE_FLOW_SMALL=0, or the failure hook
    assert [pick(n, 1, 0, 1) for n in (1, ACUT, ACUT + 1, CUTOFF + 1)] == [0] * 4  # no monitors: ppe_pick_flow_small's
    assert [pick(n, 1, 1, 0) for n in (1, ACUT, ACUT + 1, CUTOFF + 1)] == [0] * 4  # ppe_classify_flow's own batches


def test_older_planners_answer_as_before():
    lib = abi.load()
    small, comb, fps = lib.ppe_pick_flow_small, lib.ppe_pick_flow_combined, lib.ppe_pick_flow_portscan
    for n, allowed, atk in itertools.product(SIZES, (0, 1), (0, 1)):
        assert small(n, allowed, atk) == (1 if (1 <= n <= CUTOFF and allowed and not atk) else 0), (n, allowed, atk)
    assert small(1, 1, 1) == 0 and small(CUTOFF, 1, 1) == 0                     # pinned by tests/test_flow_small_plan.py
    for f, atk, on in itertools.product((0, 1, 2), (0, 1), (0, 1)):
        assert comb(f, atk, on) == (0 if f == 0 or not atk else 1 if f == 1 and on else 2), (f, atk, on)
    m = lib.ppe_flow_portscan_max()
    assert [fps(n, 1, 1) for n in (1, m, m + 1)] == [1, 1, 2] and fps(64, 0, 1) == 0 and fps(64, 1, 0) == 0
    # the two one-launch planners never both say yes
    for n, allowed, atk, ports in itertools.product(SIZES, (0, 1), (0, 1), (0, 1)):
        assert small(n, allowed, atk) + lib.ppe_pick_flow_small_attack(n, allowed, atk, ports) <= 1


def test_new_symbols_and_prototypes():
    lib = abi.load()
    names = ("ppe_classify_flow_host_ports", "ppe_pick_flow_small_attack", "DP_Attack_Object", "DP_Attack_Rule_Set",
             "DP_Attack_Del_All", "DP_Attack_Clock", "DP_Attack_Tick")
    for name in names:
        assert hasattr(lib, name) and name in abi.EXPORTS, name
    assert hasattr(lib, "ppe_launch_flow_small_attack")
    assert lib.ppe_abi_version() == 8 and abi.ABI_VERSION == 8
    hip = (ROOT / "include" / "ppe_hip.h").read_text()
    dec = (ROOT / "include" / "ppe_decode.h").read_text()
    assert "#define PPE_ABI_VERSION 8" in hip
    assert ("int ppe_classify_flow_host_ports(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out,\n"
            "                                 const ppe_cfg_t *cfg, uint32_t chunk, const uint8_t *ports);") in hip
    assert "int DP_Attack_Rule_Set(const ppe_attack_cfg_t *cfg);" in hip
    for proto in ("extern uint32_t flow_attack_able;", "struct ppe_attack;", "struct ppe_attack *DP_Attack_Object(void);",
                  "void DP_Attack_Del_All(void);", "void DP_Attack_Clock(uint64_t now_seconds);",
                  "int  DP_Attack_Tick(uint64_t now_seconds);"):
        assert proto in dec, proto
    assert "monitors are not built behind Decode" not in dec
    assert ("uint32_t ppe_pick_flow_small_attack(uint32_t n, int small_allowed, int atk_flow_attached, int ports_call);"
            in INTERNAL)
    assert "int ppe_launch_flow_small_attack(" in INTERNAL
    from ppe import Engine
    assert callable(Engine.classify_flow_host_ports)


def test_null_arguments():
    lib = abi.load()
    assert lib.ppe_classify_flow_host_ports(None, None, None, None, 0, None) == abi.PPE_EINVAL
    assert lib.DP_Attack_Rule_Set(None) == abi.PPE_EINVAL
    assert lib.ppe_classify_flow_host(None, None, None, None, 0) == abi.PPE_EINVAL


def test_the_kernel_is_a_unit_of_its_own():
    unit = (PKG / "csrc" / "ppe_kernels_flow_small_attack.hip").read_text()
    assert "#define PPE_TU_FLOW_SMALL 2" in unit and '#include "ppe_kernels.hip"' in unit
    assert "$(BUILD)/ppe_kernels_flow_small_attack.o" in (PKG / "Makefile").read_text()
    # one argument block for both kernels: the monitors' arguments travel in the classify arguments
    kern = (PKG / "csrc" / "ppe_kernels.hip").read_text()
    assert "template <int MODE, bool ATK = false>\n__global__ __launch_bounds__(PPE_FLOW_SMALL_BLOCK)" in kern


def test_decode_header_alone_and_start_values(tmp_path):
    """include/ppe_decode.h alone compiles with gcc; a program linked against the library reads flow_attack_able == 0,
    a NULL DP_Attack_Object() (no context), a tick without an object PPE_OK."""
    src = tmp_path / "atk.c"
    src.write_text('#include <stdio.h>\n#include "ppe_decode.h"\n'
                   "int main(void) {\n"
                   "    struct ppe_attack *(*obj)(void) = DP_Attack_Object;\n"
                   "    void (*clk)(uint64_t) = DP_Attack_Clock;\n"
                   "    int (*tick)(uint64_t) = DP_Attack_Tick;\n"
                   "    void (*del)(void) = DP_Attack_Del_All;\n"
                   "    clk(5);\n"
                   "    del();\n"
                   '    printf("%u %d %d %u\\n", flow_attack_able, obj() == 0, tick(6), flow_able);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "atk"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), f"-L{PKG}", "-lppe_hip",
                    f"-Wl,-rpath,{PKG}", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["0", "1", "0", "0"]


def test_decode_without_a_device_drops_everything_with_the_monitors_on():
    import pytest
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
    flow, fatk = C.c_uint32.in_dll(lib, "flow_able"), C.c_uint32.in_dll(lib, "flow_attack_able")
    assert (flow.value, fatk.value) == (0, 0)
    lib.ppe_set_output_hooks(*hooks)
    flow.value = fatk.value = 1
    try:
        mb = (abi.Mbuf * 7)()
        for i in range(7):
            mb[i].input_port = i % 4
        lib.Decode_Set_Burst(4)
        lib.DP_Attack_Clock(1000)
        for i in range(7):
            lib.Decode(C.byref(mb[i]))
        assert len(got["drop"]) == 4
        assert lib.Decode_Flush() == -19  # PPE_ENODEV
        base = C.addressof(mb)
        assert sorted((a - base) // C.sizeof(abi.Mbuf) for a in got["drop"]) == list(range(7))
        assert "fw" not in got and "punt" not in got
        assert not lib.DP_Attack_Object() and lib.DP_Attack_Tick(1001) == 0
        assert lib.DP_Attack_Rule_Set(C.byref(abi.AttackCfg())) == -19
    finally:
        flow.value = fatk.value = 0
        lib.DP_Attack_Clock(0)
        lib.ppe_set_output_hooks(HOOK(), HOOK(), HOOK())
        lib.Decode_Set_Burst(1)
