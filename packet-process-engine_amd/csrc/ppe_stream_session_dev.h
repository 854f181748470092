/* The TCP session state machine (StreamTcpPacket, dataplane/src/plugin/stream-tcp/stream-tcp.c:2982-3143) as one
 * function of (session record, packet) -> reason, for stream_tcp_midstream 0, stream_tcp_async_oneside 0 and
 * stream_tcp_reasm_enable 0, where StreamTcp is a pure verdict.  The session kernel
 * (csrc/ppe_kernels_flow_stream.hip) and the host entry ppe_stream_session_step (csrc/ppe_stream_session.cpp, which
 * the CPU tests hold against tests/stream_session_model.py) both compile this one function; line numbers are
 * stream-tcp.c's.  The branches behind midstream / async_oneside / STREAMTCP_FLAG_MIDSTREAM* / STREAMTCP_FLAG_ASYNC are
 * left out (the list with line numbers: tests/stream_session_model.py).
 *
 * Written over (a, b) = (the sender's stream, the receiver's stream): toserver client / server, toclient server /
 * client, as every branch of the reference picks its two streams; where the reference names client and server outright
 * the branch's direction says which is which. */
#ifndef PPE_STREAM_SESSION_DEV_H
#define PPE_STREAM_SESSION_DEV_H

#include <stdint.h>

#include "ppe_hip.h"

#if defined(__HIPCC__)
#define PPE_SS_FN __host__ __device__ __forceinline__
#else
#define PPE_SS_FN static inline
#endif

/* stream-tcp-private.h:10-24 */
enum { PPE_TCP_NONE = 0, PPE_TCP_LISTEN, PPE_TCP_SYN_SENT, PPE_TCP_SYN_RECV, PPE_TCP_ESTABLISHED, PPE_TCP_FIN_WAIT1,
       PPE_TCP_FIN_WAIT2, PPE_TCP_TIME_WAIT, PPE_TCP_LAST_ACK, PPE_TCP_CLOSE_WAIT, PPE_TCP_CLOSING, PPE_TCP_CLOSED };
/* session flags (stream-tcp-private.h:32-62) and stream flags (:70-89) this configuration can set */
#define PPE_SSF_SERVER_WSCALE 0x0010u
#define PPE_SSF_4WHS 0x0080u
#define PPE_SSF_EVASION 0x0100u
#define PPE_SSF_3WHS_CONFIRMED 0x1000u
#define PPE_STF_KEEPALIVE 0x0004u
#define PPE_STF_CLOSE_INITIATED 0x0010u
#define PPE_SS_NO_WS 0xffu /* PpeSsPkt.ws without the option (tcpvars.ws == NULL) */

struct PpeSsStm { uint32_t flags, wscale, isn, next_seq, last_ack, next_win, window; };
struct PpeSsn { uint32_t state, flags; PpeSsStm c, s; };
/* th: th_flags; ws: the window-scale option's shift byte or PPE_SS_NO_WS; tc: PKT_IS_TOCLIENT */
struct PpeSsPkt { uint32_t th, seq, ack, win, plen, ws, tc; };

/* The 64-B session record (PPE_FLOW_SESS_WORDS u32): [0] state | session flags << 8; [1] client stream flags |
 * wscale << 16; [2..6] client isn, next_seq, last_ack, next_win, window; [7], [8..12] the server's; [13..15] zero. */
PPE_SS_FN void ppe_ss_unpack(const uint32_t *w, PpeSsn &x) {
    x.state = w[0] & 0xffu;
    x.flags = w[0] >> 8;
    x.c = PpeSsStm{w[1] & 0xffffu, w[1] >> 16, w[2], w[3], w[4], w[5], w[6]};
    x.s = PpeSsStm{w[7] & 0xffffu, w[7] >> 16, w[8], w[9], w[10], w[11], w[12]};
}
PPE_SS_FN void ppe_ss_pack(const PpeSsn &x, uint32_t *w) {
    w[0] = x.state | (x.flags << 8);
    w[1] = x.c.flags | (x.c.wscale << 16);
    w[2] = x.c.isn, w[3] = x.c.next_seq, w[4] = x.c.last_ack, w[5] = x.c.next_win, w[6] = x.c.window;
    w[7] = x.s.flags | (x.s.wscale << 16);
    w[8] = x.s.isn, w[9] = x.s.next_seq, w[10] = x.s.last_ack, w[11] = x.s.next_win, w[12] = x.s.window;
    w[13] = w[14] = w[15] = 0u;
}

/* c ? x : y field by field (a conditional over the two structs themselves would select their addresses, which keeps the
 * record in memory instead of registers) */
PPE_SS_FN PpeSsStm ppe_ss_sel(bool c, const PpeSsStm &x, const PpeSsStm &y) {
    return PpeSsStm{c ? x.flags : y.flags, c ? x.wscale : y.wscale, c ? x.isn : y.isn, c ? x.next_seq : y.next_seq,
                    c ? x.last_ack : y.last_ack, c ? x.next_win : y.next_win, c ? x.window : y.window};
}

/* SEQ_LT .. SEQ_GEQ, stream-tcp-private.h:93-97 */
PPE_SS_FN bool ppe_seq_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }
PPE_SS_FN bool ppe_seq_leq(uint32_t a, uint32_t b) { return (int32_t)(a - b) <= 0; }
PPE_SS_FN bool ppe_seq_gt(uint32_t a, uint32_t b) { return (int32_t)(a - b) > 0; }
PPE_SS_FN bool ppe_seq_geq(uint32_t a, uint32_t b) { return (int32_t)(a - b) >= 0; }

/* StreamTcpPacket for one packet: updates x, counts through cnt(field index) every field of tcpstream_track_stat the
 * reference counts, returns 0 (STREAMTCP_OK) or the index of the reason counted last (STREAMTCP_ERR). */
template <class CNT>
PPE_SS_FN uint32_t ppe_stream_step(PpeSsn &x, const PpeSsPkt &p, CNT &&cnt) {
    const uint32_t FIN = 0x01u, SYN = 0x02u, RST = 0x04u, ACK = 0x10u;
    const uint32_t th = p.th, seq = p.seq, ack = p.ack, win = p.win, plen = p.plen, end = seq + plen;
    const bool tc = p.tc != 0u, has_ws = p.ws != PPE_SS_NO_WS;
    const uint32_t pws = (has_ws && p.ws <= 14u) ? p.ws : 0u;  /* TCP_GET_WSCALE, decode-tcp.h:103 */
    if ((th & (SYN | ACK)) == (SYN | ACK)) cnt(PPE_STC_SYN_ACK_COUNT);  /* :2989-2997 */
    else if (th & SYN) cnt(PPE_STC_SYN_COUNT);
    if (th & RST) cnt(PPE_STC_RST_COUNT);
    if (!(th & ACK) && ack != 0u) cnt(PPE_STC_PKT_BROKEN_ACK);  /* :3000-3003 */

    PpeSsStm a = ppe_ss_sel(tc, x.s, x.c), b = ppe_ss_sel(tc, x.c, x.s);
    uint32_t state = x.state, flags = x.flags, reason = 0u;
#define PPE_SS_DROP(f) do { cnt(f); reason = (f); goto done; } while (0)
#define PPE_SS_UPDATE_LAST_ACK(st, v) do { if (ppe_seq_gt((v), (st).last_ack)) (st).last_ack = (v); } while (0) /* :36-41 */
#define PPE_SS_UPDATE_NEXT_WIN(st, v) do { if (ppe_seq_gt((v), (st).next_win)) (st).next_win = (v); } while (0) /* :53-58 */
    /* StreamTcpValidateAck :73-122 against stream st */
    auto valid_ack = [&](const PpeSsStm &st) -> bool {
        if (ppe_seq_gt(ack, st.last_ack) && ppe_seq_leq(ack, st.next_win)) return true;
        if (ack == st.last_ack) return true;
        if (ppe_seq_lt(ack, st.last_ack)) {
            if (st.window != 0u && ppe_seq_lt(ack, st.last_ack - st.window)) {
                cnt(PPE_STC_PKT_INVALID_ACK);
                return false;
            }
            return true;
        }
        if (state > PPE_TCP_SYN_SENT && ppe_seq_gt(ack, st.next_win)) {
            cnt(PPE_STC_PKT_INVALID_ACK);
            return false;
        }
        if (state == PPE_TCP_SYN_SENT && tc && (th & RST) && ack == st.isn + 1u) return true;
        cnt(PPE_STC_PKT_INVALID_ACK);
        return false;
    };
    /* StreamTcpPacketIsRetransmission :1434-1454 of the sender's stream */
    auto retransmission = [&]() -> bool {
        if (plen == 0u) return false;
        if (ppe_seq_leq(end, a.last_ack) || ppe_seq_leq(end, a.next_seq)) {
            cnt(PPE_STC_PKT_RETRANSMISSION);
            return true;
        }
        return false;
    };
    /* StreamTcpPacketStateNone :237-441 (also the target of the CLOSED state's reuse, :3126) */
    auto state_none = [&]() -> uint32_t {
        if (th & RST) return PPE_STC_RST_BUT_NO_SESSION;
        if (th & FIN) return PPE_STC_FIN_BUT_NO_SESSION;
        if ((th & (SYN | ACK)) == (SYN | ACK)) return PPE_STC_MIDSTREAM_OR_ONESIDE_DISABLE;
        if (th & SYN) {  /* :328-363: client and server outright, whatever the direction */
            state = PPE_TCP_SYN_SENT;
            if (has_ws) flags |= PPE_SSF_SERVER_WSCALE;
            if (tc) {  /* (a flow whose session starts late may see its first SYN from the server's side) */
                b.isn = seq;
                b.next_seq = seq + 1u;
                a.window = win;
                if (has_ws) a.wscale = pws;
            } else {
                a.isn = seq;
                a.next_seq = seq + 1u;
                b.window = win;
                if (has_ws) b.wscale = pws;
            }
            return 0u;
        }
        if (th & ACK) return PPE_STC_MIDSTREAM_DISABLE;
        return 0u;
    };
    const bool wrong_fin_seq = ppe_seq_lt(seq, a.next_seq) || ppe_seq_gt(seq, a.last_ack + a.window);

    if (state == PPE_TCP_NONE) {  /* :3005-3008 */
        const uint32_t r = state_none();
        if (r) PPE_SS_DROP(r);
        goto done;
    }
    {
        const uint32_t sfr = th & (SYN | FIN | RST);
        /* StreamTcpPacketIsKeepAlive :2804-2844 */
        if (plen <= 1u && !sfr && ack == b.last_ack && seq == a.next_seq - 1u) {
            a.flags |= PPE_STF_KEEPALIVE;
            goto done;
        }
        const uint32_t pkt_win = win << b.wscale;
        /* StreamTcpPacketIsKeepAliveACK :2757-2798, StreamTcpClearKeepAliveFlag :2846-2859 */
        if (plen == 0u && !sfr && win != 0u && pkt_win == b.window && (b.flags & PPE_STF_KEEPALIVE) &&
            ack == b.last_ack && seq == a.next_seq) {
            b.flags &= ~PPE_STF_KEEPALIVE;
            a.flags &= ~PPE_STF_KEEPALIVE;
            goto done;
        }
        a.flags &= ~PPE_STF_KEEPALIVE;
        /* StreamTcpPacketIsWindowUpdate :2864-2905, else StreamTcpPacketIsBadWindowUpdate :2923-2972 */
        const bool est = state >= PPE_TCP_ESTABLISHED;
        const bool wupdate = est && plen == 0u && !sfr && win != 0u && pkt_win != b.window && ack == b.last_ack &&
                             seq == a.next_seq;
        if (!wupdate && est && !sfr && pkt_win < b.window && b.window - pkt_win > plen && ppe_seq_gt(ack, b.next_seq) &&
            ppe_seq_gt(seq, a.next_seq)) {
            cnt(PPE_STC_PKT_BAD_WINDOW_UPDATE);
            goto done;
        }
    }
    if (state == PPE_TCP_CLOSED) {  /* :3083-3131: a, the sender's stream, is the client's in the reuse branch */
        if (!tc && (th & SYN) && !(th & ACK) && seq != a.isn) {
            state = PPE_TCP_NONE;
            flags = 0u;
            a.flags = b.flags = 0u;
            const uint32_t r = state_none();
            if (r) PPE_SS_DROP(r);
        }
        goto done;
    }
    /* the RST branch of every state from FIN_WAIT1 on (e.g. :1726-1747) */
    if ((th & RST) && state >= PPE_TCP_FIN_WAIT1) {
        state = PPE_TCP_CLOSED;
        a.flags |= PPE_STF_CLOSE_INITIATED;
        b.flags |= PPE_STF_CLOSE_INITIATED;
        PPE_SS_UPDATE_LAST_ACK(b, ack);
        PPE_SS_UPDATE_LAST_ACK(a, seq);
        goto done;
    }
    /* StreamTcpHandleFin :135-232, from SYN_RECV and ESTABLISHED */
    if ((state == PPE_TCP_SYN_RECV || state == PPE_TCP_ESTABLISHED) && !(th & RST) && (th & FIN)) {
        if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_FIN_INVALID_ACK);
        if (wrong_fin_seq) PPE_SS_DROP(PPE_STC_FIN_OUT_OF_WINDOW);
        state = tc ? PPE_TCP_FIN_WAIT1 : PPE_TCP_CLOSE_WAIT;
        a.flags |= PPE_STF_CLOSE_INITIATED;
        if (seq == a.next_seq) a.next_seq = end;
        b.window = win << b.wscale;
        PPE_SS_UPDATE_LAST_ACK(b, ack);
        if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        goto done;
    }
    switch (state) {
    case PPE_TCP_SYN_SENT:  /* StreamTcpPacketStateSynSent :735-990 */
        if (th & RST) {     /* :747-770 (toserver: a is the client's stream) */
            if (tc || (seq == a.isn && win == 0u && ack == a.isn + 1u)) {
                state = PPE_TCP_CLOSED;
                a.flags |= PPE_STF_CLOSE_INITIATED;
                b.flags |= PPE_STF_CLOSE_INITIATED;
            }
        } else if (th & FIN) {
        } else if ((th & (SYN | ACK)) == (SYN | ACK)) {
            if ((flags & PPE_SSF_4WHS) && !tc) {  /* :776-849: a client, b server */
                if (ack != b.isn + 1u) PPE_SS_DROP(PPE_STC_WHS4_SYNACK_WITH_WRONG_ACK);
                if (seq != a.isn) PPE_SS_DROP(PPE_STC_WHS4_SYNACK_WITH_WRONG_SYN);
                state = PPE_TCP_SYN_RECV;
                a.isn = seq;
                a.next_seq = seq + 1u;
                b.window = win;
                b.last_ack = ack;
                a.last_ack = a.isn + 1u;
                b.wscale = ((flags & PPE_SSF_SERVER_WSCALE) && has_ws) ? pws : 0u;
                a.next_win = a.last_ack + a.window;  /* :835: client.window as the record holds it */
                b.next_win = b.last_ack + b.window;
                break;
            }
            if (!tc) PPE_SS_DROP(PPE_STC_WHS3_SYNACK_IN_WRONG_DIRECTION);
            /* toclient: a server, b client */
            if (ack != b.isn + 1u) PPE_SS_DROP(PPE_STC_WHS3_SYNACK_WITH_WRONG_ACK);
            /* StreamTcp3whsSynAckUpdate :443-503 */
            state = PPE_TCP_SYN_RECV;
            a.isn = seq;
            a.next_seq = seq + 1u;
            b.window = win;
            b.last_ack = ack;
            a.last_ack = a.isn + 1u;
            b.wscale = ((flags & PPE_SSF_SERVER_WSCALE) && has_ws) ? pws : 0u;
            a.next_win = a.last_ack + a.window;
            b.next_win = b.last_ack + b.window;
            flags &= ~PPE_SSF_4WHS;
        } else if (th & SYN) {  /* :867-932 */
            if (tc) {           /* a server */
                flags |= PPE_SSF_4WHS;
                a.isn = seq;
                a.next_seq = seq + 1u;
                a.window = win;
                if (has_ws) {
                    flags |= PPE_SSF_SERVER_WSCALE;
                    a.wscale = pws;
                } else {
                    flags &= ~PPE_SSF_SERVER_WSCALE;
                    a.wscale = 0u;
                }
            }
        } else if (th & ACK) {
            PPE_SS_DROP(PPE_STC_ONESIDE_DISABLE);  /* :937-941 */
        }
        break;
    case PPE_TCP_SYN_RECV:  /* StreamTcpPacketStateSynRecv :505-732 (FIN: above) */
        if (th & RST) {
            state = PPE_TCP_CLOSED;
            a.flags |= PPE_STF_CLOSE_INITIATED;
            b.flags |= PPE_STF_CLOSE_INITIATED;
        } else if ((th & (SYN | ACK)) == (SYN | ACK)) {  /* :532-561; toclient: a server, b client */
            if (!tc) PPE_SS_DROP(PPE_STC_WHS3_SYNACK_TOSERVER_SYN_RECV);
            if (ack != b.last_ack) PPE_SS_DROP(PPE_STC_WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK);
            if (seq != a.isn) PPE_SS_DROP(PPE_STC_WHS3_SYNACK_SEQ_MISMATCH);
        } else if (th & SYN) {  /* :562-577; toserver: a client */
            if (tc) PPE_SS_DROP(PPE_STC_WHS3_SYN_TOCLIENT_ON_SYN_RECV);
            if (seq != a.isn) PPE_SS_DROP(PPE_STC_WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV);
        } else if (th & ACK) {
            if ((flags & PPE_SSF_4WHS) && tc) {  /* :582-617: a server, b client */
                if (seq != a.next_seq) PPE_SS_DROP(PPE_STC_WHS4_WRONG_SEQ);
                if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_WHS4_INVALID_ACK);
                PPE_SS_UPDATE_LAST_ACK(b, ack);
                a.next_seq += plen;
                b.window = win << b.wscale;
                b.next_win = b.last_ack + b.window;
                state = PPE_TCP_ESTABLISHED;
                break;
            }
            if (tc) PPE_SS_DROP(PPE_STC_WHS3_ACK_IN_WRONG_DIR);  /* :619-632 */
            /* toserver: a client, b server */
            if (seq == a.next_seq && ack == b.next_seq) {  /* :639-669 */
                PPE_SS_UPDATE_LAST_ACK(b, ack);
                a.next_seq += plen;
                b.window = win << b.wscale;
                b.next_win = b.last_ack + b.window;
                state = PPE_TCP_ESTABLISHED;
            } else if (seq == a.next_seq) {  /* :711-717 */
                flags |= PPE_SSF_EVASION;
                PPE_SS_DROP(PPE_STC_WHS3_RIGHT_SEQ_WRONG_ACK_EVASION);
            } else {
                PPE_SS_DROP(PPE_STC_WHS3_WRONG_SEQ_WRONG_ACK);
            }
        }
        break;
    case PPE_TCP_ESTABLISHED:  /* StreamTcpPacketStateEstablished :1257-1432 (FIN: above) */
        if (th & RST) {        /* :1265-1327 */
            state = PPE_TCP_CLOSED;
            a.flags |= PPE_STF_CLOSE_INITIATED;
            b.flags |= PPE_STF_CLOSE_INITIATED;
            b.next_seq = ack;
            a.next_seq = end + (tc ? 1u : 0u);  /* :1278, :1305 */
            a.window = win << a.wscale;
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            PPE_SS_UPDATE_LAST_ACK(a, seq);
        } else if ((th & (SYN | ACK)) == (SYN | ACK)) {  /* :1336-1380; toclient: a server, b client */
            if (!tc) PPE_SS_DROP(PPE_STC_EST_SYNACK_TOSERVER);
            if (ack != b.last_ack) PPE_SS_DROP(PPE_STC_EST_SYNACK_RESEND_WITH_DIFFERENT_ACK);
            if (seq != a.isn) PPE_SS_DROP(PPE_STC_EST_SYNACK_RESEND_WITH_DIFF_SEQ);
            if (flags & PPE_SSF_3WHS_CONFIRMED) PPE_SS_DROP(PPE_STC_EST_SYNACK_RESEND);
            state = PPE_TCP_SYN_RECV;
        } else if (th & SYN) {  /* :1381-1397; toserver: a client */
            if (tc) PPE_SS_DROP(PPE_STC_EST_SYN_TOCLIENT);
            if (seq != a.isn) PPE_SS_DROP(PPE_STC_EST_SYN_RESEND_DIFF_SEQ);
            PPE_SS_DROP(PPE_STC_EST_SYN_RESEND);
        } else if (th & ACK) {  /* HandleEstablishedPacketToClient :994-1094 / ToServer :1097-1240 */
            if (tc) flags |= PPE_SSF_3WHS_CONFIRMED;
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_EST_INVALID_ACK);
            if (plen <= 1u && seq == a.next_seq - 1u) {  /* keep-alive :1019, :1110 */
            } else if (!ppe_seq_geq(end, a.last_ack)) {
                PPE_SS_DROP(PPE_STC_EST_PKT_BEFORE_LAST_ACK);
            }
            if (plen == 1u && seq == a.next_seq && a.window == 0u) break;  /* zero window probe :1046, :1185 */
            if (a.next_seq == seq) a.next_seq += plen;
            if (!ppe_seq_leq(end, a.next_win)) PPE_SS_DROP(PPE_STC_EST_PACKET_OUT_OF_WINDOW);
            b.window = win << b.wscale;
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
            PPE_SS_UPDATE_NEXT_WIN(b, b.last_ack + b.window);
        }
        break;
    case PPE_TCP_FIN_WAIT1:  /* StreamTcpPacketStateFinWait1 :1717-2111 (RST: above) */
        if (th & FIN) {      /* FIN|ACK :1748-1854 (TIME_WAIT), FIN :1855-1963 (CLOSING) */
            const bool re = retransmission();
            if (!re && wrong_fin_seq) PPE_SS_DROP(PPE_STC_FIN1_FIN_WRONG_SEQ);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_FIN1_INVALID_ACK);
            if (!re) {
                state = (th & ACK) ? PPE_TCP_TIME_WAIT : PPE_TCP_CLOSING;
                a.flags |= PPE_STF_CLOSE_INITIATED;
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
            if (a.next_seq == seq) a.next_seq += plen;
        } else if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if (th & ACK) {  /* :1970-2103 */
            const bool re = retransmission();
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_FIN1_INVALID_ACK);
            if (!re) {
                if (!ppe_seq_leq(end, a.next_win)) PPE_SS_DROP(PPE_STC_FIN1_ACK_WRONG_SEQ);
                if (seq == a.next_seq) state = PPE_TCP_FIN_WAIT2;
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
            if (a.next_seq == seq) a.next_seq += plen;
            PPE_SS_UPDATE_NEXT_WIN(b, b.last_ack + b.window);
        }
        break;
    case PPE_TCP_FIN_WAIT2:  /* StreamTcpPacketStateFinWait2 :1456-1714 (RST: above) */
        if (th & FIN) {      /* :1487-1591 */
            bool re = false;
            if (seq == a.next_seq - 1u && ack == b.last_ack) re = true;
            else if (retransmission()) re = true;
            else if (wrong_fin_seq) PPE_SS_DROP(PPE_STC_FIN2_FIN_WRONG_SEQ);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_FIN2_INVALID_ACK);
            if (!re) {
                state = PPE_TCP_TIME_WAIT;
                a.flags |= PPE_STF_CLOSE_INITIATED;
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        } else if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if (th & ACK) {  /* :1597-1707 */
            const bool re = retransmission();
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_FIN2_INVALID_ACK);
            if (!re) {
                if (!ppe_seq_leq(end, a.next_win)) PPE_SS_DROP(PPE_STC_FIN2_ACK_WRONG_SEQ);
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (a.next_seq == seq) a.next_seq += plen;
            PPE_SS_UPDATE_NEXT_WIN(b, b.last_ack + b.window);
        }
        break;
    case PPE_TCP_CLOSE_WAIT:  /* StreamTcpPacketStateCloseWait :2113-2370 (RST: above) */
        if (th & FIN) {       /* :2155-2254 */
            const bool re = retransmission();
            if (!re && wrong_fin_seq) PPE_SS_DROP(PPE_STC_CLOSEWAIT_FIN_OUT_OF_WINDOW);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_CLOSEWAIT_INVALID_ACK);
            if (!re) {
                if (tc) {  /* :2233-2238; toserver only the window, :2186-2187 */
                    state = PPE_TCP_LAST_ACK;
                    a.flags |= PPE_STF_CLOSE_INITIATED;
                }
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        } else if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if (th & ACK) {  /* :2260-2362 */
            const bool re = retransmission();
            if (plen > 0u && ppe_seq_leq(end, a.last_ack)) PPE_SS_DROP(PPE_STC_CLOSEWAIT_PKT_BEFORE_LAST_ACK);
            if (ppe_seq_gt(seq, a.last_ack + a.window)) PPE_SS_DROP(PPE_STC_CLOSEWAIT_ACK_OUT_OF_WINDOW);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_CLOSEWAIT_INVALID_ACK);
            if (!re) b.window = win << b.wscale;
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
            if (seq == a.next_seq) a.next_seq += plen;
        }
        break;
    case PPE_TCP_LAST_ACK:  /* StreamTcpPacketStateLastAck :2377-2471 (RST: above) */
        if (th & FIN) {
        } else if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if ((th & ACK) && !tc) {  /* :2418-2464: toserver only; a client, b server */
            const bool re = retransmission();
            if (seq != a.next_seq && seq != a.next_seq + 1u) PPE_SS_DROP(PPE_STC_LASTACK_ACK_WRONG_SEQ);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_LASTACK_INVALID_ACK);
            if (!re) {
                state = PPE_TCP_CLOSED;
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        }
        break;
    case PPE_TCP_CLOSING:  /* StreamTcpPacketStateClosing :2478-2607 (RST: above) */
        if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if (th & ACK) {
            const bool re = retransmission();
            if (seq != a.next_seq) PPE_SS_DROP(PPE_STC_CLOSING_ACK_WRONG_SEQ);
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_CLOSING_INVALID_ACK);
            if (!re) {
                state = PPE_TCP_TIME_WAIT;
                /* :2542 and :2585: the client's window in both directions */
                if (tc) b.window = win << b.wscale;
                else a.window = win << a.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        }
        break;
    case PPE_TCP_TIME_WAIT:  /* StreamTcpPacketStateTimeWait :2614-2752 (RST: above) */
        if (th & FIN) {
        } else if (th & SYN) {
            PPE_SS_DROP(PPE_STC_SHUTDOWN_SYN_RESEND);
        } else if (th & ACK) {
            bool re = false;
            if (retransmission()) {
                re = true;
            } else if (seq != a.next_seq && seq != a.next_seq + 1u) {
                if (tc && plen > 0u && seq == a.last_ack) break;  /* :2706-2709, the toclient side only */
                PPE_SS_DROP(PPE_STC_TIMEWAIT_ACK_WRONG_SEQ);
            }
            if (!valid_ack(b)) PPE_SS_DROP(PPE_STC_TIMEWAIT_INVALID_ACK);
            if (!re) {
                state = PPE_TCP_CLOSED;
                b.window = win << b.wscale;
            }
            PPE_SS_UPDATE_LAST_ACK(b, ack);
            if (ppe_seq_lt(b.next_seq, ack)) b.next_seq = ack;
        }
        break;
    default:  /* TCP_LISTEN: the default case :3132-3136 */
        break;
    }
done:
#undef PPE_SS_DROP
#undef PPE_SS_UPDATE_LAST_ACK
#undef PPE_SS_UPDATE_NEXT_WIN
    x.state = state;
    x.flags = flags;
    x.c = ppe_ss_sel(tc, b, a);
    x.s = ppe_ss_sel(tc, a, b);
    return reason;
}

#endif
