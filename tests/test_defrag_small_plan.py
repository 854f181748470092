"""The host side of the one-launch reassembly kernel, without a GPU: the planner that picks it (csrc/launch_plan.cpp)
on both sides of its cutoff and under each of its three conditions, the cutoff's own bounds, and the new symbols with
their prototypes."""
import ctypes as C
import re
from pathlib import Path

from ppe import abi

ROOT = Path(__file__).resolve().parent.parent
INTERNAL = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()


def cutoff():
    return int(re.search(r"#define PPE_DEFRAG_SMALL_CUTOFF (\d+)u", INTERNAL).group(1))


def test_planner_picks_the_one_launch_kernel_up_to_the_cutoff():
    lib = abi.load()
    pick, c = lib.ppe_pick_defrag_small, cutoff()
    below = sorted({1, 2, c - 1, c} - {0})
    assert [pick(n, 1, 0) for n in below] == [1] * len(below)
    assert [pick(n, 1, 0) for n in (c + 1, 8000, 65536, 1 << 24)] == [0] * 4    # above the cutoff: six launches
    assert [pick(n, 1, 0) for n in (63, 64, 65)] == [1 if n <= c else 0 for n in (63, 64, 65)]
    assert pick(0, 1, 0) == 0
    assert [pick(n, 0, 0) for n in (1, 64, c, c + 1)] == [0] * 4                # a table created under PPE_DEFRAG_SMALL=0
    assert [pick(n, 1, 1) for n in (1, 64, c, c + 1)] == [0] * 4                # the PPE_DF_LOOK_FAIL hook armed
    assert [pick(n, 0, 1) for n in (1, c)] == [0, 0]


def test_cutoff_conditions():
    """One fragment per thread in the per-fragment phases: the cutoff cannot pass the workgroup."""
    c = cutoff()
    block = int(re.search(r"#define PPE_DEFRAG_SMALL_BLOCK (\d+)", INTERNAL).group(1))
    assert block in (256, 1024) and 1 <= c <= block


def test_new_symbols_resolve():
    lib = abi.load()
    for name in ("ppe_defrag_host", "ppe_defrag_launch_info", "ppe_pick_defrag_small"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert lib.ppe_abi_version() == 8
    assert lib.ppe_defrag_host(None, None, None, 0) == abi.PPE_EINVAL
    assert lib.ppe_defrag_launch_info(None, None, None) == abi.PPE_EINVAL
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    assert ("int  ppe_defrag_host(ppe_defrag_t *d, const ppe_frag_batch_t *in, const ppe_defrag_out_t *out, "
            "uint32_t chunk);") in hdr
    assert "int  ppe_defrag_launch_info(ppe_defrag_t *d, uint32_t *kind, uint32_t *launches);" in hdr
    assert "uint32_t ppe_pick_defrag_small(uint32_t n, int small_allowed, int look_fail_armed);" in INTERNAL


def test_the_kernel_is_a_unit_of_its_own():
    """csrc/ppe_defrag_small.hip is csrc/ppe_defrag.hip again under its macro, and the library's build lists it."""
    pkg = ROOT / "packet-process-engine_amd"
    unit = (pkg / "csrc" / "ppe_defrag_small.hip").read_text()
    assert "#define PPE_TU_DEFRAG_SMALL 1" in unit and '#include "ppe_defrag.hip"' in unit
    assert "$(BUILD)/ppe_defrag_small.o" in (pkg / "Makefile").read_text()
    assert hasattr(abi.load(), "ppe_launch_defrag_small")


def test_decode_symbols_and_prototypes():
    lib = abi.load()
    for name in ("DP_Defrag_Clock", "DP_Defrag_Age", "DP_Defrag_Table"):
        assert hasattr(lib, name) and name in abi.EXPORTS
    assert C.c_uint32.in_dll(lib, "defrag_able").value == 0
    assert C.c_uint32.in_dll(lib, "defrag_cache_max").value == 8
    dec = (ROOT / "include" / "ppe_decode.h").read_text()
    for proto in ("extern uint32_t defrag_able;", "extern uint32_t defrag_cache_max;",
                  "void DP_Defrag_Clock(uint64_t now_seconds);",
                  "int  DP_Defrag_Age(uint64_t now_seconds, uint64_t *dropped);",
                  "struct ppe_defrag_table *DP_Defrag_Table(void);", "#define PKT_FRAG_REASM_COMP (1 << 3)"):
        assert proto in dec


def test_decode_header_globals_and_start_values(tmp_path):
    """include/ppe_decode.h alone compiles with gcc, and a program linked against the library reads the start values:
    reassembly off, a cache of 8; aging without a table is PPE_OK with nothing dropped, and there is no table."""
    import subprocess
    src = tmp_path / "df.c"
    src.write_text('#include <stdio.h>\n#include "ppe_decode.h"\n'
                   "int main(void) {\n"
                   "    void (*clk)(uint64_t) = DP_Defrag_Clock;\n"
                   "    int (*age)(uint64_t, uint64_t *) = DP_Defrag_Age;\n"
                   "    uint64_t dropped = 7;\n"
                   "    clk(5);\n"
                   "    const int rc = age(1000, &dropped);\n"
                   '    printf("%u %u %d %llu %d %d %d\\n", defrag_able, defrag_cache_max, rc, (unsigned long long)dropped,\n'
                   "           age(1000, 0), DP_Defrag_Table() == 0, PKT_FRAG_REASM_COMP);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "df"
    lib = ROOT / "packet-process-engine_amd"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), f"-L{lib}", "-lppe_hip",
                    f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["0", "8", "0", "0", "0", "1", "8"]


def test_decode_without_a_device_drops_everything_with_reassembly_on():
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
    able = C.c_uint32.in_dll(lib, "defrag_able")
    lib.ppe_set_output_hooks(*hooks)
    able.value = 1
    try:
        mb = (abi.Mbuf * 7)()
        lib.Decode_Set_Burst(4)
        lib.DP_Defrag_Clock(1000)
        for i in range(7):
            lib.Decode(C.byref(mb[i]))
        assert len(got["drop"]) == 4
        assert lib.Decode_Flush() == -19  # PPE_ENODEV
        base = C.addressof(mb)
        assert sorted((a - base) // C.sizeof(abi.Mbuf) for a in got["drop"]) == list(range(7))
        assert "fw" not in got and "punt" not in got
        dropped = C.c_uint64(3)
        assert lib.DP_Defrag_Age(2000, C.byref(dropped)) == 0 and dropped.value == 0
        assert not lib.DP_Defrag_Table()
    finally:
        able.value = 0
        lib.ppe_set_output_hooks(HOOK(), HOOK(), HOOK())
        lib.Decode_Set_Burst(4096)


def test_the_planner_is_the_one_decision_point():
    """ppe_defrag asks ppe_pick_defrag_small_upto with its table's value, which PPE_DEFRAG_SMALL sets through
    ppe_defrag_small_upto_from_env: unset or 1 the cutoff, 0 none, N > 1 min(N, the workgroup)."""
    lib = abi.load()
    upto, env, c = lib.ppe_pick_defrag_small_upto, lib.ppe_defrag_small_upto_from_env, cutoff()
    block = int(re.search(r"#define PPE_DEFRAG_SMALL_BLOCK (\d+)", INTERNAL).group(1))
    assert [env(v) for v in (-1, 0, 1, 2, 17, block, block + 1, 1 << 20)] == [c, 0, c, 2, 17, block, block, block]
    for n in (0, 1, c, c + 1, 17, block, block + 1):
        for allowed in (0, 1):
            for armed in (0, 1):
                assert lib.ppe_pick_defrag_small(n, allowed, armed) == upto(n, c if allowed else 0, armed)
    assert [upto(n, block, 0) for n in (0, 1, 17, block, block + 1)] == [0, 1, 1, 1, 0]
    assert [upto(n, 1 << 20, 0) for n in (block, block + 1)] == [1, 0]        # never past the workgroup
    assert [upto(n, block, 1) for n in (1, block)] == [0, 0]                   # the hook armed
    assert [upto(n, 0, 0) for n in (1, c)] == [0, 0]
    src = (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_defrag.hip").read_text()
    assert src.count("ppe_pick_defrag_small_upto(a.n, d->small_upto, a.look_fail_wg != ~0u)") == 1
    assert "uint32_t ppe_pick_defrag_small_upto(uint32_t n, uint32_t upto, int look_fail_armed);" in INTERNAL
