#!/usr/bin/env python3
"""Generate tests/golden/ref_stream_session_v1.npz: the reference's own StreamTcpPacket over the known-answer scripts
and the generated conversations of tests/stream_session_corpus.py, packet by packet.

Run by hand where the reference tree is present.  In a temporary directory outside the repository it puts copies of the
reference's stream-tcp.c, stream-tcp-private.h and decode-statistic.h, unmodified, beside stand-in headers written here
(sec-common.h, oct-common.h, mbuf.h, shm.h, flow.h, stream-tcp.h, stream-tcp-session.h, stream-tcp-reassemble.h,
dp_attack.h: the few types, macros and prototypes stream-tcp.c reads, with the TCP header kept in host order) and a
driver, compiles them with gcc, sets stream_tcp_reasm_enable = 0 (midstream and async_oneside are 0 in the source) and
runs every packet through StreamTcpPacket.  A flow's session is what StreamTcpNewSession returns: here calloc'd, the
engine's zero-record definition.  StreamTcpReassembleHandleSegment is the stand-in of its first lines
(stream-tcp-reassemble.c:460-464: reassembly off returns OK with the packet).

Frozen per sequence: the packets, the return value of every packet, the fields of struct tcpstream_track_stat it
changed (up to four indices), the counters at the end and every flow's final session.  Only this output is committed;
nothing compiled from the reference and none of its text is."""
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "tests")]
import stream_session_corpus as sc  # noqa: E402
import stream_session_model as m  # noqa: E402

REF = Path("/root/reference/dataplane/src")
OUT = Path(__file__).resolve().parent / "ref_stream_session_v1.npz"

COMMON = r"""
#ifndef STANDIN_COMMON_H
#define STANDIN_COMMON_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <inttypes.h>
#define LOGDBG(mask, str...)
#define LOCAL_CPU_ID 0
#ifndef TRUE
#define TRUE 1
#define FALSE 0
#endif
#define SEC_OK 1
#define SEC_NO 0
#define TH_FIN 0x01
#define TH_SYN 0x02
#define TH_RST 0x04
#define TH_PUSH 0x08
#define TH_ACK 0x10
#define TH_URG 0x20
#define TCP_WSCALE_MAX 14
typedef struct { uint32_t th_seq, th_ack; uint16_t th_win; uint8_t th_flags; } TCPHdr;   /* host order */
typedef struct { uint8_t *data; } TCPOpt;
typedef struct { TCPOpt *ws; } TCPVars;
typedef struct { void *protoctx; uint32_t input_port; } flow_item_t;
typedef struct mbuf_s {
    void *transport_header;
    uint32_t flags;
    uint32_t payload_len;
    TCPVars tcpvars;
    void *flow;
} mbuf_t;
#define PKT_TO_SERVER (1 << 0)
#define PKT_TO_CLIENT (1 << 1)
#define PKT_HAS_WS (1 << 6)
#define PKT_IS_TCP(p) 1
#define PKT_IS_TOSERVER(p) (((p)->flags & PKT_TO_SERVER))
#define PKT_IS_TOCLIENT(p) (((p)->flags & PKT_TO_CLIENT))
#define TCP_GET_SEQ(p) (((TCPHdr *)((p)->transport_header))->th_seq)
#define TCP_GET_ACK(p) (((TCPHdr *)((p)->transport_header))->th_ack)
#define TCP_GET_WINDOW(p) (((TCPHdr *)((p)->transport_header))->th_win)
/* the option's shift byte, 0 without the option or above the maximum (what decode-tcp.h's macro of this name yields) */
static inline uint8_t standin_wscale(const mbuf_t *p) {
    if (!p->tcpvars.ws) return 0;
    const uint8_t v = p->tcpvars.ws->data[0];
    return v <= TCP_WSCALE_MAX ? v : 0;
}
#define TCP_GET_WSCALE(p) standin_wscale(p)
#endif
"""
STREAM_TCP_H = r"""
#ifndef STANDIN_STREAM_TCP_H
#define STANDIN_STREAM_TCP_H
#include "sec-common.h"
#include "stream-tcp-private.h"
#define STREAMTCP_OK 0
#define STREAMTCP_ERR 1
#define STREAMTCP_CACHE 2
static inline void StreamTcpPacketSwitchDir(TcpSession *ssn, mbuf_t *m) { (void)ssn; m->flags ^= PKT_TO_SERVER | PKT_TO_CLIENT; }
extern uint32_t stream_tcp_track_enable, stream_tcp_reasm_enable, stream_tcp_midstream, stream_tcp_async_oneside;
uint32_t StreamTcpPacket(mbuf_t *mbuf, mbuf_t **reasm_m);
TcpSession *StreamTcpNewSession(mbuf_t *mbuf);
void StreamTcpReturnStreamSegments(TcpStream *stream);
uint32_t StreamTcpReassembleHandleSegment(TcpSession *ssn, TcpStream *stream, mbuf_t *m, mbuf_t **reasm_m);
void DP_Attack_SynCountFins(mbuf_t *m);
uint32_t StreamTcpSessionInit(void);
#endif
"""
DRIVER = r"""
#include "stream-tcp.h"
#include "decode-statistic.h"
pkt_stat g_stat;
pkt_stat *pktstat[1] = {&g_stat};
TcpSession *StreamTcpNewSession(mbuf_t *mbuf) {
    TcpSession *s = calloc(1, sizeof *s);
    ((flow_item_t *)mbuf->flow)->protoctx = s;
    s->state = TCP_NONE;
    return s;
}
void StreamTcpReturnStreamSegments(TcpStream *stream) { (void)stream; }
void DP_Attack_SynCountFins(mbuf_t *m) { (void)m; }
uint32_t StreamTcpSessionInit(void) { return SEC_OK; }
uint32_t StreamTcpReassembleHandleSegment(TcpSession *ssn, TcpStream *stream, mbuf_t *m, mbuf_t **reasm_m) {
    (void)ssn; (void)stream;
    if (!stream_tcp_reasm_enable) { *reasm_m = m; return STREAMTCP_OK; }
    abort();
}
/* in: n, nflows, then n x {flow, th, seq, ack, win, plen, ws (0xff none), toclient}; out: n x {ret, changed fields},
 * 58 counters (u64 as two u32), nflows x 16 session words */
int main(int argc, char **argv) {
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[2];
    if (argc < 3 || !fi || !fo || fread(hd, 4, 2, fi) != 2) return 2;
    const uint32_t n = hd[0], nf = hd[1];
    flow_item_t *flows = calloc(nf, sizeof *flows);
    stream_tcp_reasm_enable = 0;
    if (stream_tcp_midstream || stream_tcp_async_oneside || !stream_tcp_track_enable) return 3;
    const size_t NF = sizeof(struct tcpstream_track_stat) / 8;
    uint64_t *cur = (uint64_t *)&g_stat.tcpstreamtrackstat, prev[64];
    if (NF != 58) return 4;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[8];
        if (fread(w, 4, 8, fi) != 8) return 5;
        TCPHdr h = {w[2], w[3], (uint16_t)w[4], (uint8_t)w[1]};
        uint8_t wsb = (uint8_t)w[6];
        TCPOpt opt = {&wsb};
        mbuf_t mb, *out = NULL;
        memset(&mb, 0, sizeof mb);
        mb.transport_header = &h;
        mb.flags = w[7] ? PKT_TO_CLIENT : PKT_TO_SERVER;
        mb.payload_len = w[5];
        mb.tcpvars.ws = w[6] == 0xff ? NULL : &opt;
        mb.flow = &flows[w[0]];
        memcpy(prev, cur, NF * 8);
        uint32_t r[2] = {StreamTcpPacket(&mb, &out), 0xffffffffu};
        int k = 0;
        for (size_t f = 0; f < NF && k < 4; f++)
            if (cur[f] != prev[f]) { r[1] = (r[1] & ~(0xffu << (8 * k))) | ((uint32_t)f << (8 * k)); k++; }
        fwrite(r, 4, 2, fo);
    }
    fwrite(cur, 8, NF, fo);
    for (uint32_t f = 0; f < nf; f++) {
        uint32_t w[16] = {0};
        TcpSession *s = flows[f].protoctx;
        if (s) {
            w[0] = s->state; w[1] = s->flags;
            TcpStream *st[2] = {&s->client, &s->server};
            for (int j = 0; j < 2; j++) {
                uint32_t *q = w + 2 + 7 * j;
                q[0] = st[j]->flags; q[1] = st[j]->wscale; q[2] = st[j]->isn; q[3] = st[j]->next_seq;
                q[4] = st[j]->last_ack; q[5] = st[j]->next_win; q[6] = st[j]->window;
            }
        }
        fwrite(w, 4, 16, fo);
    }
    fclose(fo);
    return 0;
}
"""


def sequences():
    """name -> [(flow, Pkt)]: every trigger and conversation on a flow of its own for each ISN pair, a flag sweep
    behind the way into every state, and the generated conversations."""
    ka, f = [], 0
    for cisn, sisn in sc.ISNS:
        for _, pre, steps in sc.TRIGGERS:
            ka += [(f, p) for p in sc.packets(pre + steps, cisn, sisn)]
            f += 1
        for conv in sc.CONVERSATIONS + [pre + [sc.c(sc.S, 0)] for pre in sc.SHUTDOWN_STATES]:
            ka += [(f, p) for p in sc.packets(conv, cisn, sisn)]
            f += 1
    sweep, f = [], 0
    for pre, _ in sc.PREFIX_STATE:
        for side in "cs":
            for fl in range(64):
                for dseq, dack in ((0, 0), (1, 1), (1, 2), (2, 1)):
                    tail = [(side, fl, dseq, dack, 1000, 0, None), (side, fl | 0x10, dseq, dack, 999, 3, 7)]
                    sweep += [(f, p) for p in sc.packets(pre + tail, 1000, 5000)]
                    f += 1
    return {"known": ka, "sweep": sweep, "generated": sc.generate()}


def run_reference(exe, seq, td):
    nf = max(f for f, _ in seq) + 1
    words = np.array([[f, p.flags, p.seq, p.ack, p.win, p.plen, 0xFF if p.ws is None else p.ws, int(p.toclient)]
                      for f, p in seq], np.uint32)
    fin, fout = Path(td) / "in.bin", Path(td) / "out.bin"
    fin.write_bytes(np.array([len(seq), nf], np.uint32).tobytes() + words.tobytes())
    subprocess.run([str(exe), str(fin), str(fout)], check=True)
    raw = fout.read_bytes()
    n = len(seq)
    res = np.frombuffer(raw[:8 * n], np.uint32).reshape(n, 2)
    cnt = np.frombuffer(raw[8 * n:8 * n + 8 * 58], np.uint64)
    ssn = np.frombuffer(raw[8 * n + 8 * 58:], np.uint32).reshape(nf, 16)
    return words, res[:, 0].astype(np.uint8), res[:, 1].copy(), cnt.copy(), ssn.copy()


def main():
    with tempfile.TemporaryDirectory() as td:
        t = Path(td)
        for src in ("plugin/stream-tcp/stream-tcp.c", "plugin/stream-tcp/stream-tcp-private.h",
                    "decode/decode-statistic.h"):
            shutil.copy(REF / src, t / Path(src).name)
        (t / "sec-common.h").write_text(COMMON)
        (t / "stream-tcp.h").write_text(STREAM_TCP_H)
        for name in ("oct-common.h", "mbuf.h", "shm.h", "flow.h", "stream-tcp-session.h", "stream-tcp-reassemble.h",
                     "dp_attack.h"):
            (t / name).write_text('#include "sec-common.h"\n')
        (t / "driver.c").write_text(DRIVER)
        exe = t / "ref_stream"
        subprocess.run(["gcc", "-O1", "-std=gnu99", "-w", f"-I{t}", str(t / "stream-tcp.c"), str(t / "driver.c"), "-o",
                        str(exe)], check=True)
        out = {}
        for name, seq in sequences().items():
            words, ret, changed, cnt, ssn = run_reference(exe, seq, td)
            # (the packets are frozen for the smaller sequences only: generate() rebuilds its own from the seed)
            if name != "generated":
                out[f"{name}_pkt"] = words.astype(np.uint32)
            out[f"{name}_n"] = np.array([len(seq)], np.uint32)
            out[f"{name}_ret"], out[f"{name}_changed"], out[f"{name}_counters"], out[f"{name}_sessions"] = ret, changed, cnt, ssn
            print(name, len(seq), "packets,", int(ret.sum()), "rejected")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
