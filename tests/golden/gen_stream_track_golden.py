#!/usr/bin/env python3
"""Generate tests/golden/tcpstream_stat_ex_v1.txt: the text the reference's `show tcpstream statistic` would print for
a fixed vector over all 58 fields of struct tcpstream_track_stat and the setting the session path runs under (track
enabled, reasm disabled).

Run where the reference tree is present.  As gen_tcpstream_golden.py, it walks dp_show_tcpstream_stat in
dataplane/src/common/dp_cmd.c statement by statement: the two `%s` enable / disable lines, then each
`x += pktstat[i]->tcpstream{track,reasm}stat.<FIELD>` sum followed by its `sprintf(ptr, "<fmt>", x)`, evaluated with
field i of the struct (ppe.abi.STREAM_TRACK_COUNTERS, the struct's order) = 5000 + 31 i and every reassembly field 0.
Only the resulting output text is committed (a golden vector); the reference file itself is not."""
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "packet-process-engine_amd")]
from ppe.abi import STREAM_TRACK_COUNTERS  # noqa: E402

REF = Path("/root/reference/dataplane/src/common/dp_cmd.c")
OUT = Path(__file__).resolve().parent
COUNTS = {name: 5000 + 31 * i for i, name in enumerate(STREAM_TRACK_COUNTERS)}
CFG = {"stream_tcp_track_enable": 1, "stream_tcp_reasm_enable": 0}

PAT = re.compile(r'(?P<reset>\bx\s*=\s*0;)|x\s*\+=\s*pktstat\[i\]->tcpstream(?P<kind>track|reasm)stat\.(?P<field>[A-Za-z_0-9]+);'
                 r'|sprintf\(\(void \*\)ptr,\s*"(?P<fmt>(?:[^"\\]|\\.)*)"\s*'
                 r'(?:,\s*(?P<var>[a-z_]+)\s*\?\s*"(?P<yes>[^"]*)"\s*:\s*"(?P<no>[^"]*)"|(?P<arg>,\s*x))?\)')


def body(src: str, name: str) -> str:
    i = src.index(f"void {name}()")
    return src[i:src.index("\n}\n", i)]


def eval_show(text: str) -> str:
    out, x, seen = [], 0, set()
    for m in PAT.finditer(text):
        if m.group("reset"):
            x = 0
        elif m.group("field"):
            if m.group("kind") == "track":
                x += COUNTS[m.group("field")]  # (a field the struct does not have: KeyError)
                seen.add(m.group("field"))
        else:
            fmt = m.group("fmt").replace("\\n", "\n").replace("%ld", "%d")
            if m.group("var"):
                out.append(fmt % (m.group("yes") if CFG[m.group("var")] else m.group("no")))
            else:
                out.append(fmt % x if m.group("arg") else fmt)
    print("fields the show function does not print:", sorted(set(COUNTS) - seen))
    return "".join(out)


def main():
    src = REF.read_text(errors="replace")
    (OUT / "tcpstream_stat_ex_v1.txt").write_text(eval_show(body(src, "dp_show_tcpstream_stat")))
    print("wrote", OUT / "tcpstream_stat_ex_v1.txt")


if __name__ == "__main__":
    main()
