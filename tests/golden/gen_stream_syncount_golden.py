#!/usr/bin/env python3
"""Generate tests/golden/ref_stream_syncount_v1.npz: for every packet of gen_stream_session_golden.py's three sequences
(the known answers, the flag sweep, the generated conversations: the same 39,282 packets), whether the reference's own
StreamTcpPacket called DP_Attack_SynCountFins on it (stream-tcp.c:608, :660).

Run by hand where the reference tree is present.  It is gen_stream_session_golden.py's build with one change: the
stand-in DP_Attack_SynCountFins counts its calls, and the driver writes the count of each packet into bits 8-15 of the
packet's return word.  The reference's files are copied unmodified into a temporary directory, compiled there and
thrown away; only this output is committed.

stream-tcp-session.c (StreamTcp_Flow_ResRelease, :61-77) is not compiled: beside the stand-ins it needs the memory
pools and the boot-memory allocator (mem_pool_alloc, Mem_Pool_Cfg, cvmx_bootmem_alloc_named), none of which the session
machine touches.  Its rule, protoctx != NULL && state <= TCP_SYN_RECV, rests on the hand-derived cases of
tests/test_flow_stream_attack_model.py."""
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE)]
import gen_stream_session_golden as base  # noqa: E402

OUT = HERE / "ref_stream_syncount_v1.npz"

OLD_FINS = "void DP_Attack_SynCountFins(mbuf_t *m) { (void)m; }"
NEW_FINS = "static uint32_t g_fins;\nvoid DP_Attack_SynCountFins(mbuf_t *m) { (void)m; g_fins++; }"
OLD_CALL = "uint32_t r[2] = {StreamTcpPacket(&mb, &out), 0xffffffffu};"
NEW_CALL = "g_fins = 0;\n        uint32_t r[2] = {StreamTcpPacket(&mb, &out), 0xffffffffu};\n        r[0] |= g_fins << 8;"
assert base.DRIVER.count(OLD_FINS) == 1 and base.DRIVER.count(OLD_CALL) == 1
DRIVER = base.DRIVER.replace(OLD_FINS, NEW_FINS).replace(OLD_CALL, NEW_CALL)


def main():
    with tempfile.TemporaryDirectory() as td:
        t = Path(td)
        for src in ("plugin/stream-tcp/stream-tcp.c", "plugin/stream-tcp/stream-tcp-private.h",
                    "decode/decode-statistic.h"):
            shutil.copy(base.REF / src, t / Path(src).name)
        (t / "sec-common.h").write_text(base.COMMON)
        (t / "stream-tcp.h").write_text(base.STREAM_TCP_H)
        for name in ("oct-common.h", "mbuf.h", "shm.h", "flow.h", "stream-tcp-session.h", "stream-tcp-reassemble.h",
                     "dp_attack.h"):
            (t / name).write_text('#include "sec-common.h"\n')
        (t / "driver.c").write_text(DRIVER)
        exe = t / "ref_stream"
        subprocess.run(["gcc", "-O1", "-std=gnu99", "-w", f"-I{t}", str(t / "stream-tcp.c"), str(t / "driver.c"), "-o",
                        str(exe)], check=True)
        out, total = {}, 0
        for name, seq in base.sequences().items():
            nf = max(f for f, _ in seq) + 1
            words = np.array([[f, p.flags, p.seq, p.ack, p.win, p.plen, 0xFF if p.ws is None else p.ws, int(p.toclient)]
                              for f, p in seq], np.uint32)
            fin, fout = t / "in.bin", t / "out.bin"
            fin.write_bytes(np.array([len(seq), nf], np.uint32).tobytes() + words.tobytes())
            subprocess.run([str(exe), str(fin), str(fout)], check=True)
            res = np.frombuffer(fout.read_bytes()[:8 * len(seq)], np.uint32).reshape(len(seq), 2)
            out[f"{name}_ret"] = (res[:, 0] & 0xFF).astype(np.uint8)
            out[f"{name}_fins"] = (res[:, 0] >> 8).astype(np.uint8)
            total += len(seq)
            print(name, len(seq), "packets,", int(out[f"{name}_fins"].sum()), "calls")
        out["n"] = np.array([total], np.uint32)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
