/*
 * ppe_decode.h — PPE-compatible decoder / plugin / log-hook surface over the GPU engine.
 *
 * Reference interfaces this replaces:
 *   void Decode(mbuf_t *m)                                dataplane/src/decode/decode.c:19-28
 *   DECODE_OK / DECODE_DROP / DECODE_DONE                 dataplane/src/decode/decode.h:7-9
 *   mbuf_t parse fields (eth_dst/src, ipv4, sport, dport, proto, vlan_idx, payload_len, timestamp, flags)
 *                                                         dataplane/src/include/mbuf.h:23-87
 *   PluginModule / plugin_modules[PLUGIN_SIZE]            dataplane/src/plugin/plugin-mod/plugin.h:9-19, plugin.c:8
 *   reg_fw_alert / DP_Log_Func                            dataplane/src/common/dp_log.c:12-31
 *   int DP_Acl_Lookup(mbuf_t *)                           dataplane/src/flow/flow.c:232
 *
 * The reference decodes one mbuf per call on the calling core and has finished with it when Decode returns
 * (decode.c:13-28).  So does this Decode by default: the burst size is 1, and Decode(m) classifies m on the GPU and
 * delivers it before it returns.  A caller that wants GPU-sized batches opts in with Decode_Set_Burst(n): Decode(m)
 * then appends the mbuf to the calling thread's own burst (one per thread, as the reference's per-core mainloop),
 * classified when it reaches n entries or when that thread calls Decode_Flush() (or exits).  Either way the
 * verdict is delivered exactly as the reference does — output_fw_proc(m) / output_drop_proc(m) hooks, with
 * DP_Log_Func(m) on the drop reasons the reference logs — and the mbuf's parse fields are filled in.
 * Every classification runs on the GPU; there is no CPU decode path.
 */
#ifndef PPE_DECODE_H
#define PPE_DECODE_H

#include <stdint.h>
#include "ppe_acl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DECODE_OK   0
#define DECODE_DROP 1
#define DECODE_DONE 2

/* mbuf flags (dataplane/src/decode/decode.h:12-21) */
#define PKT_IP_FRAG    (1 << 1)
#define PKT_FRAG_REASM_COMP (1 << 3)   /* a reassembled datagram's mbuf (decode.h:14, decode-defrag.c:274) */
#define PKT_TO_SERVER  (1 << 4)
#define PKT_TO_CLIENT  (1 << 5)
#define PKT_HAS_FLOW   (1 << 8)

#ifndef PPE_HAVE_CVMX
/* the Octeon SDK's 64-bit work-queue buffer word (cvmx-packet.h); a build that includes cvmx.h defines
 * PPE_HAVE_CVMX and uses the SDK's own type */
typedef union {
    uint64_t u64;
} cvmx_buf_ptr_t;
#endif

#ifndef __DECODE_TCP_H__
/* dataplane/src/decode/decode-tcp.h:24-46 (only the types mbuf_t embeds) */
typedef struct TCPOpt_ {
    uint8_t type;
    uint8_t len;
    uint8_t *data;
} TCPOpt;

typedef struct TCPVars_ {
    TCPOpt tcp_opts[1];
    TCPOpt *ws;                /* the window-scale option DecodeTCPOptions recorded (decode-tcp.c:61-70), filled by
                                  Decode from the kernel's option parse; NULL (as allocated) when there is none */
} TCPVars;
#define TCP_OPTS tcpvars.tcp_opts  /* m->TCP_OPTS[0], decode-tcp.c:66-68 */
#endif

typedef void (*FreeAlState)(void *s);

typedef struct {
    uint32_t sip;
    uint32_t dip;
} ipv4_tuple_t;

/* The reference's mbuf_t, field for field in the reference's order (dataplane/src/include/mbuf.h:23-87), so
 * oct_rx_process_work-style producers (dataplane/src/platform/oct-rxtx.c:190-206: magic_flag, pkt_space,
 * packet_ptr, input_port, pkt_totallen, pkt_ptr, tag, timestamp) compile against it unchanged; on LP64 every
 * reference field keeps its reference offset (sizeof of the reference part = 232 B, the memset of
 * oct-rxtx.c:192).  The engine's results are appended after `tag`. */
typedef struct m_buf_ {
    uint32_t magic_flag;       /* MBUF_MAGIC_NUM                                                 */
    uint8_t pkt_space;         /* PKTBUF_HW / PKTBUF_SW                                          */
    uint8_t flow_log;
    uint16_t frag_len;
    cvmx_buf_ptr_t packet_ptr;
    struct m_buf_ *next;
    void *pkt_ptr;             /* start of the L2 frame                                         */
    void *ethh;                /* set on decode                                                  */
    void *vlanh;
    void *network_header;
    void *transport_header;
    uint32_t input_port;
    uint8_t eth_dst[6];
    uint8_t eth_src[6];
    ipv4_tuple_t ipv4;
    uint16_t sport;
    uint16_t dport;
    uint8_t proto;
    uint8_t vlan_idx;
    uint16_t payload_len;
    uint16_t vlan_id;          /* never written by the reference decoder             */
    uint16_t defrag_id;
    uint64_t timestamp;        /* seconds since 1970; the ACL time window is checked against it */
    void *payload;
    union {
        TCPVars tcpvars;
    };
    uint16_t frag_offset;
    uint16_t tcp_reasm_overlap;
    uint32_t pkt_totallen;     /* wire length                                                   */
    uint32_t flags;
    uint32_t fcb_hash;
    void *fcb;
    struct m_buf_ *fragments;
    void *flow;
    struct m_buf_ *tcp_seg_raw;
    struct m_buf_ *tcp_seg_raw_tail;
    struct m_buf_ *tcp_seg_reassem;
    void *alState;
    FreeAlState FreeState;
    uint32_t tag;
    /* engine results (no reference counterpart) */
    uint32_t ppe_verdict;      /* status | action << 8 | flags << 16 (ppe_hip.h)                 */
    uint32_t ppe_flow_hash;    /* flow_hashfn value (bucket = & 0xFFFF, dataplane/src/flow/flow.c:76-79) */
    int32_t ppe_acl_hit;       /* lowest matching rule index or -1                               */
    void *user;
} mbuf_t;

#define MBUF_MAGIC_NUM 0xab00ab00 /* dataplane/src/include/mbuf.h:91 */
#define PKTBUF_HW 1
#define PKTBUF_SW 2

/* Output hooks (the reference's output_fw_proc / output_drop_proc, dataplane/src/output/output.c:106,151).
 * punt: fragments for Defrag (decode-ipv4.c:234) and packets whose headers exceed the header window. */
typedef void (*ppe_output_fn)(mbuf_t *m);
void ppe_set_output_hooks(ppe_output_fn fw, ppe_output_fn drop, ppe_output_fn punt);

/* config knobs pushed by the manager in the reference (dp_cmd.c:37 unsupport_proto_action, flow.c:26 syn_check) */
extern uint32_t unsupport_proto_action;
extern uint32_t syn_check;
/* StreamTcp's settings (stream-tcp.c:16,20-21), read per classify call like syn_check.  All start at 0 here (tracking
 * OFF; the reference starts with stream_tcp_track_enable = 1): see ppe_stream_tcp_set in ppe_hip.h */
extern uint32_t stream_tcp_track_enable;
extern uint32_t stream_tcp_midstream;
extern uint32_t stream_tcp_async_oneside;
/* The port-scan detector behind Decode (PortScan_Detect on every flow miss, flow.c:215-230; the stateless path treats
 * every packet as one), named as in the reference (dp_portscan.c:9-11, dp_attack.c:25) and read per classify call.
 * Start values: portscan_able 0 (OFF: the verdicts stay those without the detector; the reference starts with 1),
 * portscan_action 0 (drop), portscan_exception_freq 50, flood_hold_time 600.  With portscan_able == 1 the first
 * flush creates the table (PORTSCAN_ITEM_NUM = 100,000 records) and every burst runs the detector in burst order
 * through ppe_classify_host_ordered (ppe_hip.h); across threads the order is the order in which the flushes take the
 * engine.  A packet it drops (status PPE_ST_PORTSCAN_DROP) goes to the drop hook without DP_Log_Func (flow.c:216-230
 * logs nothing), with the fields the TCP / UDP decoders wrote and without PKT_HAS_FLOW / PKT_TO_SERVER.  Setting
 * portscan_able back to 0 keeps the table and its records, and the verdicts are again those without it.  The land /
 * flood monitors run ahead of the flow table only (flow_attack_able below): the stateless host paths have none. */
extern uint32_t portscan_able;
extern uint32_t portscan_action;
extern uint32_t portscan_exception_freq;
extern uint32_t flood_hold_time;
/* cvmx_get_cycle() and OCT_TIME_SECONDS_SINCE1970 (dp_portscan.c:158-198) for the bursts flushed afterwards, by
 * value; 1e9 cycles are one second.  Both start at 0.  mbuf->timestamp is what the hold test reads (:145). */
void DP_PortScan_Clock(uint64_t now_cycles, uint64_t now_seconds);
/* PortScan_timeout (dp_portscan.c:43-93) at now_cycles; *freed (may be NULL) = records freed.  PPE_OK without a table */
int  DP_PortScan_Age(uint64_t now_cycles, uint64_t *freed);
/* the detector's table for ppe_portscan_info / _dump / ppe_format_pkt_stat_ps / ppe_format_fw_config (ppe_hip.h);
 * NULL before the first flush with portscan_able == 1 and after DP_Acl_Rule_Release */
struct ppe_portscan_table;
struct ppe_portscan_table *DP_PortScan_Table(void);

/* The flow table behind Decode (FlowHandlePacket with FlowGetFlowFromHash, flow.c:181-310), read per classify call.
 * Start values: flow_able 0 (OFF: Decode is the stateless path, every packet its flow's first; the reference has no
 * such switch, its Decode always goes through the table), flow_item_num 100000 (MEM_POOL_FLOW_NODE_NUM), read when
 * the table is created.  With flow_able == 1 the first flush creates the context's table (flow_item_num flows) and
 * every burst goes through ppe_classify_flow_host_ports (ppe_hip.h; with no monitors attached it is
 * ppe_classify_flow_host byte for byte) in burst order, a burst larger than the first in chunks; across threads the order is the order in which the flushes take the engine.  Then a packet whose flow exists
 * is forwarded without an ACL lookup (ppe_acl_hit == -1), replies carry PKT_TO_CLIENT | PKT_HAS_FLOW, the creating
 * direction PKT_TO_SERVER | PKT_HAS_FLOW, and a packet without a flow (ACL drop, FLOW_TCP_NO_SYN_FIRST, or
 * PPE_ST_FLOW_NOMEM when the pool is empty, which goes to the drop hook without DP_Log_Func, flow.c:124-129) carries
 * neither.  There is no host flow object: m->flow stays as it was.  The table is read through the shim's context:
 * ppe_flow_info / ppe_flow_dump / ppe_format_flow_stat on ppe_compat_ctx().  Setting flow_able back to 0 keeps the
 * table and its flows; DP_Acl_Rule_Release destroys it with the context.
 * flow_able == 1 together with portscan_able == 1 or stream_tcp_track_enable is refused (portscan_able is the stateless
 * path's switch, every packet a miss; the flow table's detector is flow_portscan_able below; the TCP session machine is
 * not built): the flush fails with PPE_ENOTSUP before any state changes and every mbuf of the burst goes to the drop
 * hook, as for any classify step that cannot run. */
extern uint32_t flow_able;
extern uint32_t flow_item_num;
/* The port-scan detector on the flow table's misses (PortScan_Detect inside FlowGetFlowFromHash, flow.c:196-243: after
 * syn_check, before the ACL; a packet that finds its flow never reaches it), read per classify call.  Start value 0.
 * With flow_able == 1, flow_portscan_able == 1, portscan_able == 0 and stream tracking off, the first flush creates the
 * shim's port-scan table (the one portscan_able uses, 100,000 records) and attaches it to the flow table's path
 * (ppe_flow_portscan_attach, ppe_hip.h); every flush takes portscan_action, portscan_exception_freq, flood_hold_time and
 * DP_PortScan_Clock's values and goes through ppe_classify_flow_host_ports.  DP_PortScan_Age and DP_PortScan_Table work on
 * that table.  A packet the detector drops (PPE_ST_PORTSCAN_DROP) goes to the drop hook without DP_Log_Func, without
 * PKT_HAS_FLOW and without a direction flag.  With flow_able == 0 it has no effect.  Setting it back to 0 detaches the
 * table and keeps its records. */
extern uint32_t flow_portscan_able;
/* The land, SYN-flood, SYN-count and UDP-flood monitors ahead of the flow table (DecodeIPV4 / DecodeTCP call them before
 * FlowHandlePacket, decode-ipv4.c:141-149, decode-tcp.c:162-173; the SYN-count monitor counts in FlowAdd,
 * flow.c:151-154), read per classify call.  Start value 0.  It has an effect only with flow_able == 1, as
 * flow_portscan_able: the reference runs its monitors ahead of the flow table only, and the stateless host paths
 * (flow_able == 0, with or without portscan_able) still have none.
 * The shim keeps one monitor object (ppe_attack_*, ppe_hip.h), created on first use with all-zero rules
 * (DP_Attack_Del_All's state) and hold_seconds = flood_hold_time.  While flow_able == 1 && flow_attack_able == 1 it is
 * attached to the flow table's path (ppe_flow_attack_attach); otherwise it is detached and keeps its rules and state.
 * Every flush with flow_able == 1 builds one input-port byte per mbuf from m->input_port (the kernels use port & 3; a
 * reassembled datagram carries its chain head's) and goes through ppe_classify_flow_host_ports; flood_hold_time is read
 * per flush, as the detector path reads it.  With flow_portscan_able == 1 as well the shim turns ppe_flow_combine on for
 * its context and the burst runs the combined path (monitors, then the detector on the survivors' misses); the switch
 * then stays on for ppe_compat_ctx() (with only one of the two attached it changes nothing).
 * A packet a monitor drops (statuses 25-28) goes to the drop hook without DP_Log_Func (decode-ipv4.c:145-148 and
 * decode-tcp.c:162-172 log nothing), without PKT_HAS_FLOW, without a direction flag and with ports 0: it never reached
 * FlowHandlePacket.  flow_able == 1 with portscan_able == 1 or stream tracking is refused as above, whatever this is.
 * Not built: the monitors on the stateless host paths, per-fragment counting (a reassembled datagram counts once), the
 * /data/protection.rul parser (DP_Attack_Rule_Set in ppe_hip.h takes the parsed rules). */
extern uint32_t flow_attack_able;
/* The entry points below take the shim's lock, so they order with other threads' flushes. */
/* the shim's monitor object for ppe_attack_info / ppe_format_attack_stat / ppe_attack_clear_stat (ppe_hip.h): created if
 * a context exists (DP_Acl_Rule_Init), else NULL; NULL again after DP_Acl_Rule_Release, which destroys it before its
 * context */
struct ppe_attack;
struct ppe_attack *DP_Attack_Object(void);
/* DP_Attack_Del_All (dp_attack.c): every rule back to zero; the counts, holds and drop totals stay */
void DP_Attack_Del_All(void);
/* OCT_TIME_SECONDS_SINCE1970 for the bursts flushed afterwards, by value (the hold arming reads it).  Starts at 0. */
void DP_Attack_Clock(uint64_t now_seconds);
/* DP_Attack_Info_Update (dp_attack.c:712-748; once a second in the reference): pps = accum, accum = 0, expired holds
 * cleared; sets the clock too.  PPE_OK without an object */
int  DP_Attack_Tick(uint64_t now_seconds);
/* FLOW_UPDATE_TIMESTAMP's clock (seconds) for the bursts flushed afterwards, by value.  Starts at 0; with
 * flow_able == 0 the classify calls keep now_seconds = 0. */
void DP_Flow_Clock(uint64_t now_seconds);
/* FlowAgeTimeoutCB (flow.c:391-467) at now_seconds with FLOW_MAX_TIMEOUT = 20: flows idle for more than 20 s are
 * deleted; *deleted (may be NULL) = their number.  PPE_OK with 0 deleted without a table. */
int  DP_Flow_Age(uint64_t now_seconds, uint64_t *deleted);

/* Defrag behind Decode (decode-ipv4.c:102-125: no fragment leaves DecodeIPV4 unhandled), read per flush.  Start values:
 * defrag_able 0 (OFF: Decode hands every fragment to the punt hook; the reference has no such switch, it is always
 * on), defrag_cache_max 8 (decode-defrag.c:24), read when the table is created.  With defrag_able == 1 a flush
 *   - classifies the burst as without it, on whichever path the other switches select;
 *   - runs its fragments (status PPE_ST_FRAG) through ppe_defrag_host (ppe_hip.h) in burst order, whole frames
 *     gathered from pkt_ptr / pkt_totallen, now_seconds = DP_Defrag_Clock's; the first such flush creates the table
 *     (DEFRAG_FCB_MAX = 1,024 FCBs of defrag_cache_max fragments);
 *   - holds a cached fragment (PPE_DF_CACHED, and PPE_DF_SETUP_ERR): no hook is called for it
 *     (decode-defrag.c:391-392, 281-283).  The caller keeps the mbuf object alive until a hook gets it; pkt_ptr is
 *     not read again (the device store holds the copy, as PACKET_HW2SW's);
 *   - hands a fragment Defrag drops (FCB_FULL, HW2SW_ERR, DELETED, CACHE_FULL, DEFRAG_ERR) to the drop hook, with
 *     DP_Log_Func only where decode-defrag.c calls it (:436, cache full; here before the drop hook, as for every
 *     logged drop, so the hook may free the mbuf);
 *   - builds, for a fragment that completes its datagram, the reassembled mbuf as Frag_defrag_setup / _reasm leave it
 *     (:164-220, 241-276): zeroed, PKTBUF_SW, MBUF_MAGIC_NUM, input_port of the chain's head, timestamp 0, pkt_ptr the
 *     reassembled frame, pkt_totallen its length, flags PKT_FRAG_REASM_COMP, fragments = the caller's mbufs in chain
 *     order linked through next.  The burst's datagrams are classified from their frames like any other mbuf, as a
 *     second burst behind the first in the order of their completing fragments, on the same path.  At burst 1 that is
 *     the reference's order (Defrag's datagram goes on into DecodeTCP / DecodeUDP / the flow table before the next
 *     packet); at a larger burst a datagram counts as arriving behind its burst's last packet;
 *   - calls the hooks in burst order with no lock held: the datagram's one call (fw, drop with DP_Log_Func as for
 *     any packet, or punt) takes the place of its completing fragment.  The reassembled mbuf and its frame are the
 *     shim's and valid during the call; the chain belongs to the hook (output.c:122-170 forwards or frees it).
 * Decode_Flush then returns the number of hook calls.  Setting defrag_able back to 0 keeps the table and what it
 * holds (DP_Defrag_Age still works).  When the defrag step or the datagrams' classify step fails, every undelivered
 * mbuf of the burst goes to the drop hook and so does everything the table held; the table is destroyed and created
 * afresh at the next flush.  Not built: per-fragment monitor counting, teardrop as an action, zero-copy for pinned
 * frames. */
extern uint32_t defrag_able;
extern uint32_t defrag_cache_max;
/* FCB_UPDATE_TIMESTAMP's clock (seconds) for the bursts flushed afterwards, by value.  Starts at 0. */
void DP_Defrag_Clock(uint64_t now_seconds);
/* Frag_defrag_timeout (decode-defrag.c:490-551) at now_seconds with FRAG_MAX_TIMEOUT = 20: completed FCBs and those
 * idle for more than 20 s are freed; every fragment they held goes to the drop hook (no DP_Log_Func); *dropped (may
 * be NULL) = their number.  PPE_OK with 0 dropped without a table. */
int  DP_Defrag_Age(uint64_t now_seconds, uint64_t *dropped);
/* the FCB table for ppe_defrag_info / ppe_format_pkt_stat_ex / ppe_format_flow_stat_ex (ppe_hip.h); NULL before the
 * first flush with defrag_able == 1 that carries a fragment and after DP_Acl_Rule_Release (which hands every held
 * mbuf to the drop hook first) */
struct ppe_defrag_table;
struct ppe_defrag_table *DP_Defrag_Table(void);

void Decode(mbuf_t *m);
/* Classify every mbuf the calling thread has queued; returns the number delivered through the output hooks, or a
 * negative PPE_E* code when the GPU step failed, in which case every queued mbuf was handed to the drop hook (the
 * reference ends every undelivered packet in output_drop_proc).  Hooks run with no engine lock held, so a hook
 * may call Decode() again (e.g. a punt hook feeding reassembled datagrams back). */
int  Decode_Flush(void);
/* Burst size at which Decode() flushes automatically: 1 (the default) = synchronous, the reference's contract; a
 * larger n queues up to n mbufs per thread (the caller then calls Decode_Flush() at its batch boundaries).  May be
 * changed at any time; it applies to every thread's next Decode().  n = 0 is ignored. */
void Decode_Set_Burst(uint32_t n);

/* Batch form of DP_Acl_Lookup over already-decoded mbufs (ACL_RULE_ACTION_FW / _DROP per mbuf). */
int  DP_Acl_Lookup_Burst(mbuf_t **m, uint32_t n, int *actions);
int  DP_Acl_Lookup(mbuf_t *m);

/* ---- plugin ABI (dataplane/src/plugin/plugin-mod/plugin.h:9-19) ---- */
typedef enum {
    PLUGIN_STREAMTCP,
    PLUGIN_SIZE,
} PluginId;

typedef struct {
    char *name;
    int (*Init)(void);
    int (*Func)(mbuf_t *m);
} PluginModule;

extern PluginModule plugin_modules[PLUGIN_SIZE];

/* ---- drop-log hook (dataplane/src/common/dp_log.c:12-31) ---- */
typedef int (*fw_alert)(void *);
void reg_fw_alert(fw_alert fun);
void DP_Log_Func(mbuf_t *m);

/* engine context behind the compat layer (created by DP_Acl_Rule_Init) */
struct ppe_ctx;
struct ppe_ctx *ppe_compat_ctx(void);

#ifdef __cplusplus
}
#endif
#endif /* PPE_DECODE_H */
