"""Python model of StreamTcp's first-packet verdict on the stateless classify path (ppe_stream_tcp_set), for the tests.

The oracle stops at FLOW_PROC_OK (oracle/ppe_oracle.c:459-461): it answers what the engine answers with tracking
off.  This model takes the oracle's result for a batch, the header bytes and a setting, and rewrites exactly the
packets the reference's StreamTcp would see first (TCP, ACL consulted, ACL forwarded: flow.c:311-320), by the rules of
StreamTcpPacketStateNone (dataplane/src/plugin/stream-tcp/stream-tcp.c:237-441) and the counters of StreamTcpPacket
(:2989-3003).  Citations are to the reference's stream-tcp.c unless another file is named."""
import numpy as np

from ppe import abi
from ppe.abi import ST

TH_FIN, TH_SYN, TH_RST, TH_ACK = 0x01, 0x02, 0x04, 0x10
OFF = dict(track=0, midstream=0, async_oneside=0)


def first_packet_status(flags: int, midstream: int, async_oneside: int) -> int:
    """StreamTcpPacketStateNone for th_flags `flags` (track on): the resulting engine status, first match wins."""
    if flags & TH_RST:                                   # :243-248 STREAM_RST_BUT_NO_SESSION, STREAMTCP_ERR
        return ST["STREAM_RST_NO_SESSION"]
    if flags & TH_FIN:                                   # :249-254 STREAM_FIN_BUT_NO_SESSION
        return ST["STREAM_FIN_NO_SESSION"]
    if flags & (TH_SYN | TH_ACK) == (TH_SYN | TH_ACK):   # :255-261
        if midstream == 0 and async_oneside == 0:
            return ST["STREAM_MIDSTREAM_ONESIDE_OFF"]
        return ST["ACL_FW"]                              # :263-294 session picked up, STREAMTCP_OK
    if flags & TH_SYN:                                   # :296-362 new session, STREAMTCP_OK
        return ST["ACL_FW"]
    if flags & TH_ACK:                                   # :364-370
        if midstream == 0:
            return ST["STREAM_MIDSTREAM_OFF"]
        raise NotImplementedError("ACK-only midstream pickup enters segment reassembly (:371-432): PPE_ENOTSUP")
    return ST["ACL_FW"]                                  # :434-437 nothing to do


def th_fields(hdr: np.ndarray, verdict: np.ndarray):
    """(th_flags, th_ack) of every packet from the header bytes: L4 at 14, plus 4 if PPE_F_VLAN, plus ihl * 4; flags
    at +13, the 32-bit ack field at +8 (garbage where the packet has no TCP header: callers mask)."""
    n, stride = hdr.shape
    fl = verdict >> 16
    l3 = 14 + 4 * ((fl & abi.F_VLAN) != 0).astype(np.int64)
    rows = np.arange(n)
    ihl = (hdr[rows, np.minimum(l3, stride - 1)] & 0xF).astype(np.int64) * 4
    l4 = l3 + ihl
    g = lambda off: hdr[rows, np.minimum(l4 + off, stride - 1)].astype(np.uint32)  # noqa: E731
    ack = (g(8) << 24) | (g(9) << 16) | (g(10) << 8) | g(11)
    return g(13), ack


def expected(ref: dict, hdr: np.ndarray, cfg: dict) -> dict:
    """ref = the oracle's classify_batch result (verdict, flow_hash, acl_hit, tuple, counters) for hdr; cfg = dict(track,
    midstream, async_oneside).  Returns verdict / flow_hash / acl_hit / tuple, `counters` (ppe_counters_t as a dict)
    and `stream` (ppe_stream_counters_t as a dict).  A stream drop keeps acl_hit, the flow hash, the tuple and every
    flag; in ppe_counters_t it had already counted ACL_FW (flow.c:240) and FLOW_PROC_OK (flow.c:309) and now counts
    OUT_DROP instead of OUT_FW; FLOW_PROC_FAIL is not counted."""
    verdict = ref["verdict"].copy()
    cnt = dict(zip(abi.COUNTERS, (int(x) for x in ref["counters"])))
    sc = dict.fromkeys(abi.STREAM_COUNTERS, 0)
    if cfg.get("track"):
        st, fl = verdict & 0xFF, verdict >> 16
        need = abi.F_TCP | abi.F_ACL
        seen = (st == ST["ACL_FW"]) & ((fl & need) == need)
        flags, ack = th_fields(hdr, verdict)
        reason = {ST["STREAM_RST_NO_SESSION"]: "rst_but_no_session", ST["STREAM_FIN_NO_SESSION"]: "fin_but_no_session",
                  ST["STREAM_MIDSTREAM_ONESIDE_OFF"]: "midstream_or_oneside_disable",
                  ST["STREAM_MIDSTREAM_OFF"]: "midstream_disable"}
        for i in np.flatnonzero(seen):
            f = int(flags[i])
            # counted first, :2989-3003
            if f & (TH_SYN | TH_ACK) == (TH_SYN | TH_ACK):
                sc["syn_ack_count"] += 1
            elif f & TH_SYN:
                sc["syn_count"] += 1
            if f & TH_RST:
                sc["rst_count"] += 1
            if not (f & TH_ACK) and int(ack[i]) != 0:
                sc["pkt_broken_ack"] += 1
            s = first_packet_status(f, cfg.get("midstream", 0), cfg.get("async_oneside", 0))
            if s != ST["ACL_FW"]:  # STREAMTCP_ERR -> output_drop_proc (flow.c:316-319)
                verdict[i] = s | (abi.ACT_DROP << 8) | (int(fl[i]) << 16)
                sc[reason[s]] += 1
                cnt["out_fw"] -= 1
                cnt["out_drop"] += 1
    return dict(verdict=verdict, flow_hash=ref["flow_hash"], acl_hit=ref["acl_hit"], tuple=ref["tuple"], counters=cnt,
                stream=sc)


def lists(verdict: np.ndarray) -> dict:
    """The compacted outputs a verdict array implies (include/ppe_hip.h ppe_result_t): fw_idx / drop_idx per tile with
    -7 (the tests' fill) in unused slots, tile_cnt, the partition list and its compact form part8."""
    n = len(verdict)
    act = ((verdict >> 8) & 0xFF).astype(np.int64)
    fw = np.full(n, -7, np.int64)
    dr = np.full(n, -7, np.int64)
    part = np.zeros(n, np.uint32)
    tc = np.zeros((n + 63) // 64, np.uint32)
    for t in range((n + 63) // 64):
        lo, hi = 64 * t, min(n, 64 * t + 64)
        f = np.flatnonzero(act[lo:hi] == 0) + lo
        d = np.flatnonzero(act[lo:hi] == 1) + lo
        p = np.flatnonzero(act[lo:hi] == 2) + lo
        fw[lo:lo + len(f)] = f
        dr[lo:lo + len(d)] = d
        tc[t] = len(f) | (len(d) << 8) | (len(p) << 16)
        part[lo:hi] = np.concatenate([f, p | (2 << 30), d | (1 << 30)]).astype(np.uint32)
    part8 = ((part & 63) | ((part >> 30) << 6)).astype(np.uint8)
    return dict(fw_idx=fw.astype(np.int32).view(np.uint32), drop_idx=dr.astype(np.int32).view(np.uint32), tile_cnt=tc,
                part_idx=part, part8=part8)


def packed(verdict: np.ndarray, flow_hash: np.ndarray, acl_hit: np.ndarray) -> np.ndarray:
    """ppe_result_t.packed (PPE_PACKED_*): hash | status << 32 | action << 37 | flags (six) << 39 | (hit + 1) << 45."""
    v = verdict.astype(np.uint64)
    hi = (v & np.uint64(31)) | (((v >> np.uint64(8)) & np.uint64(3)) << np.uint64(5)) | \
         (((v >> np.uint64(16)) & np.uint64(63)) << np.uint64(7)) | \
         ((acl_hit.astype(np.int64) + 1).astype(np.uint64) << np.uint64(13))
    return flow_hash.astype(np.uint64) | (hi << np.uint64(32))
