/*
 * ppe_hip.h — C ABI of the MI355X-native decode + 5-tuple ACL classify engine.
 *
 * One call classifies a whole batch of packets on the GPU: Ethernet → [one VLAN tag] → IPv4 → TCP|UDP header parse,
 * 5-tuple extraction, the symmetric TluHash flow hash and the first-match ACL lookup, with per-reason counters and
 * per-tile ballot-compacted FW/DROP index lists.  It replaces, for a whole batch at once, the reference's per-mbuf
 * hot path:
 *
 *   Decode(mbuf)                         dataplane/src/decode/decode.c:19-28
 *   └ DecodeEthernet / DecodeVLAN        dataplane/src/decode/decode-ethernet.c:23-115, decode-vlan.c:23-89
 *   └ DecodeIPV4 / DecodeIPV4Packet      dataplane/src/decode/decode-ipv4.c:27-247
 *   └ DecodeUDP / DecodeTCP              dataplane/src/decode/decode-udp.c:16-71, decode-tcp.c:135-222
 *   └ FlowHandlePacket → flow_hashfn     dataplane/src/flow/flow.c:181-245,271-292, flow/tluhash.h:7-35
 *     └ (first packet) syn_check, DP_Acl_Lookup   dataplane/src/flow/flow.c:204-243
 *
 * Stateless semantics: every packet is treated as the first packet of its flow (flow-table miss), which is the
 * reference behaviour for the unique-flow inputs of the benchmark configs.  Fragments and
 * packets whose headers extend past the header window are PUNTed to the host (status PPE_ST_FRAG /
 * PPE_ST_WINDOW_PUNT); the reference hands fragments to Defrag (decode-ipv4.c:216-239), out of scope here.
 *
 * All pointers in ppe_batch_t / ppe_result_t passed to ppe_classify() are DEVICE pointers (hipMalloc / torch
 * cuda tensors) on the context's device.  ppe_classify_host() takes host pointers and runs the pipelined
 * H2D → classify → D2H path.  Functions return 0 or a negative errno-style code (PPE_E*).
 * Thread-compatible per context: one host thread per context (as one run-to-completion core per mainloop).
 */
#ifndef PPE_HIP_H
#define PPE_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "ppe_acl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ppe_tuning_t grew to 20 B (batches_per_launch) and mbuf_t (ppe_decode.h) took the reference's field layout;
 * 3: ppe_tuple's word 3 carries the TCP window-scale option offset (bits 9-15); 4: ppe_result_t.part8;
 * 5: the tuple carries a fragment's Defrag fields and the option-past-the-window bit; strides 64..256;
 * 6: ppe_acl_stats_t cut fields; 7: ppe_rules_stage / _publish; 8: ppe_result_t.packed (8-B verdict + flow hash +
 * ACL hit); additive within 8 (no existing struct or value changes): the StreamTcp first-packet verdict
 * (ppe_stream_tcp_*, statuses 20-23, ppe_stream_counters_*, ppe_format_tcpstream_stat), off until set; the port-scan
 * detector (ppe_portscan_*, status 24, ppe_format_pkt_stat_ps, ppe_format_fw_config), off until a table is attached;
 * the land / SYN-flood / UDP-flood monitors (ppe_attack_*, statuses 25-28, ppe_format_attack_stat,
 * ppe_format_pkt_stat_atk), off until an object is attached; ppe_classify_host_ordered and
 * ppe_portscan_prepass_info; ppe_classify_flow_host and ppe_flow_launch_info; ppe_flow_portscan_attach, _max, _rounds;
 * ppe_flow_combine; ppe_classify_flow_host_ports (the monitors on host flow batches, ppe_flow_launch_info kind 4);
 * the TCP session state machine on the flow path (ppe_flow_stream_attach, _max, _dump, ppe_stream_track_counters_*,
 * ppe_format_tcpstream_stat_ex, status 29, ppe_flow_launch_info kind 5), off until attached */
#define PPE_ABI_VERSION 8

/* error codes (negative return values) */
#define PPE_OK       0
#define PPE_EINVAL  (-22)
#define PPE_ENOMEM  (-12)
#define PPE_ENODEV  (-19)
#define PPE_EIO     (-5)
#define PPE_ENOTSUP (-95)

/* ---- per-packet verdict word: status (bits 0-7) | action (bits 8-15) | flags (bits 16-31) ---- */
/* status = the terminal reason, one per reference drop/ok reason (dataplane/src/decode/decode-statistic.h:239-327) */
enum ppe_status {
    PPE_ST_ACL_FW = 0,            /* ACL passed (hit with action FW, or default FW)      STAT_ACL_FW        flow.c:240   */
    PPE_ST_ACL_DROP = 1,          /* ACL drop                                             STAT_ACL_DROP      flow.c:234   */
    PPE_ST_L2_HEADER_ERR = 2,     /* len<14, or all-zero dst/src MAC                      decode-ethernet.c:29-54      */
    PPE_ST_L2_UNSUPPORT = 3,      /* ethertype not 0x0800/0x8100/0x9100                   decode-ethernet.c:102-111    */
    PPE_ST_VLAN_HEADER_ERR = 4,   /* len<4 at a VLAN tag                                  decode-vlan.c:28-33          */
    PPE_ST_VLAN_LAYER_EXCEED = 5, /* second VLAN tag                                      decode-vlan.c:35-39          */
    PPE_ST_VLAN_UNSUPPORT = 6,    /* inner type not 0x0800/0x8100/0x9100                  decode-vlan.c:76-84          */
    PPE_ST_IPV4_HEADER_ERR = 7,   /* len<20 or ihl*4<20                                   decode-ipv4.c:30-48          */
    PPE_ST_IPV4_VERSION_ERR = 8,  /* version != 4                                         decode-ipv4.c:36-40          */
    PPE_ST_IPV4_LEN_ERR = 9,      /* ip_len<ihl*4 or len<ip_len                           decode-ipv4.c:50-60          */
    PPE_ST_FRAG_LEN_ERR = 10,     /* fragment with zero payload                           decode-ipv4.c:227-232        */
    PPE_ST_FRAG = 11,             /* fragment → Defrag (PUNT to host)                     decode-ipv4.c:216-239        */
    PPE_ST_IPV4_UNSUPPORT = 12,   /* protocol not TCP/UDP                                 decode-ipv4.c:347-357        */
    PPE_ST_UDP_HEADER_ERR = 13,   /* l4len<8                                              decode-udp.c:18-22           */
    PPE_ST_UDP_LEN_ERR = 14,      /* uh_len != l4len                                      decode-udp.c:26-36           */
    PPE_ST_TCP_HEADER_ERR = 15,   /* l4len<20                                             decode-tcp.c:140-144         */
    PPE_ST_TCP_LEN_ERR = 16,      /* l4len<hlen or (u8)(hlen-20)>40                        decode-tcp.c:148-160         */
    PPE_ST_FLOW_TCP_NO_SYN_FIRST = 17, /* flow miss, TCP without SYN, syn_check on        flow.c:204-214               */
    PPE_ST_WINDOW_PUNT = 18,      /* needed header bytes lie beyond the header window (engine-specific PUNT)          */
    PPE_ST_FLOW_NOMEM = 19,       /* flow table: ACL passed but the flow pool is exhausted  STAT_FLOW_NODE_NOMEM flow.c:127 */
    /* StreamTcp's verdict for a packet without a session (StreamTcpPacketStateNone, dataplane/src/plugin/stream-tcp/
     * stream-tcp.c:237-441), only with ppe_stream_tcp_set tracking on: the ACL forwarded the packet, then
     * STREAMTCP_ERR → output_drop_proc (flow.c:311-320).  acl_hit, PPE_F_ACL and the tuple keep the ACL's results. */
    PPE_ST_STREAM_RST_NO_SESSION = 20,        /* RST                        STREAM_RST_BUT_NO_SESSION  stream-tcp.c:243-248 */
    PPE_ST_STREAM_FIN_NO_SESSION = 21,        /* FIN                        STREAM_FIN_BUT_NO_SESSION  stream-tcp.c:249-254 */
    PPE_ST_STREAM_MIDSTREAM_ONESIDE_OFF = 22, /* SYN|ACK, midstream and async_oneside both 0           stream-tcp.c:255-261 */
    PPE_ST_STREAM_MIDSTREAM_OFF = 23,         /* ACK without SYN, midstream 0                           stream-tcp.c:364-370 */
    /* PortScan_Detect (dataplane/src/attack/dp_portscan.c:231-272) answered NOMEM, DETECTED or HOLD with
     * portscan_action 0, only with a table attached (ppe_portscan_attach): STAT_ATTACK_PORTSCAN_DROP and return NULL
     * before the ACL (flow.c:216-230), so acl_hit is -1 and PPE_F_ACL clear; flow hash, tuple and other flags stay. */
    PPE_ST_PORTSCAN_DROP = 24,
    /* PPE_ST__COUNT keeps its value: the statuses a context without a port-scan table produces (0-23; bindings and
     * tables sized by it stay valid).  PPE_ST__END counts every status, PPE_ST_PORTSCAN_DROP included. */
    PPE_ST__COUNT = 24,
    PPE_ST__END = 25,
    /* The attack monitors of dataplane/src/attack/dp_attack.c, only with an object attached (ppe_attack_attach).  All
     * four drop before the L4 decoders finish and before FlowHandlePacket: acl_hit -1, PPE_F_ACL and PPE_F_L4 clear,
     * flow hash 0, tuple word 2 zero, word 3 = proto | vlan << 8; PPE_F_TCP | PPE_F_SYN set on 25-27, neither on 28. */
    PPE_ST_ATTACK_LAND = 25,      /* TCP SYN with sip == dip       STAT_ATTACK_LAND           dp_attack.c:464-484 */
    PPE_ST_ATTACK_SYNFLOOD = 26,  /* SYN-flood hold or speed       STAT_ATTACK_SYNFLOOD_DROP  dp_attack.c:637-670 */
    PPE_ST_ATTACK_SYNCOUNT = 27,  /* syncount above syn_count      STAT_ATTACK_SYNCOUNT       dp_attack.c:673-685 */
    PPE_ST_ATTACK_UDPFLOOD = 28,  /* UDP-flood hold or speed       STAT_ATTACK_UDPFLOOD_DROP  dp_attack.c:582-634 */
    PPE_ST__ALL = 29,             /* every status, the monitors' included (PPE_ST__END keeps its value) */
    /* the TCP session machine on the flow path (ppe_flow_stream_attach): StreamTcp rejected the packet in a state other
     * than "no session" (stream-tcp.c:3009-3140 -> STREAMTCP_ERR -> output_drop_proc, flow.c:311-320).  The packet had
     * its flow: hash, tuple, acl_hit and every flag stay (PPE_F_FLOW, the direction, PPE_F_NEWFLOW included), and bits
     * 10-15 of the flags carry the reason (PPE_VERDICT_STREAM_REASON).  PPE_ST__COUNT, _END and _ALL keep their values */
    PPE_ST_STREAM_TRACK_DROP = 29,
    PPE_ST__ALL2 = 30             /* every status, this one included */
};

enum ppe_action { PPE_ACT_FW = 0, PPE_ACT_DROP = 1, PPE_ACT_PUNT = 2 };

#define PPE_F_VLAN   0x0001u   /* one VLAN tag decoded (mbuf->vlan_idx == 1)          */
#define PPE_F_L4     0x0002u   /* 5-tuple valid (reached FlowHandlePacket)            */
#define PPE_F_TCP    0x0004u
#define PPE_F_SYN    0x0008u   /* TCP SYN flag set                                    */
#define PPE_F_ACL    0x0010u   /* ACL consulted (acl_hit is its result)               */
#define PPE_F_FRAG   0x0020u   /* IPv4 fragment seen                                  */
#define PPE_F_FLOW   0x0040u   /* flow table: the packet has a flow (PKT_HAS_FLOW, flow.c:307)              */
#define PPE_F_TOCLIENT 0x0080u /* flow table: PKT_TO_CLIENT (clear with PPE_F_FLOW: PKT_TO_SERVER, flow.c:248-301) */
#define PPE_F_NEWFLOW 0x0100u  /* flow table: this packet created its flow (FlowAdd, flow.c:120-158)             */

#define PPE_PART_INDEX(e)  ((e) & 0x3fffffffu)   /* partition-layout entry → packet index                */
#define PPE_PART_ACTION(e) ((e) >> 30)           /* partition-layout entry → enum ppe_action             */
#define PPE_PART8_OFFSET(e) ((e) & 63u)          /* compact entry (part8) → packet index - 64 × tile      */
#define PPE_PART8_ACTION(e) ((e) >> 6)           /* compact entry (part8) → enum ppe_action               */

/* tuple word 3: the window-scale option DecodeTCPOptions records (decode-tcp.c:61-70), as its byte offset from the
 * TCP header (0 = none); OPT_PAST: none was found before the option parse needed a byte past the header window
 * (stride), so the answer needs a wider window (the reference reads the whole option space) */
#define PPE_TUPLE_WS(w3)      (((w3) >> 9) & 63u)
#define PPE_TUPLE_OPT_PAST    (1u << 15)

#define PPE_VERDICT_STATUS(v) ((v) & 0xffu)
#define PPE_VERDICT_ACTION(v) (((v) >> 8) & 0xffu)
#define PPE_VERDICT_FLAGS(v)  ((v) >> 16)
/* status PPE_ST_STREAM_TRACK_DROP only: the reason, an enum ppe_stream_track_counter from 9 up (bits 10-15 of the
 * flags, which no other path sets; zero for every other status) */
#define PPE_F_STREAM_REASON_SHIFT 10u
#define PPE_VERDICT_STREAM_REASON(v) (((v) >> 26) & 63u)

/* ---- packed result (ppe_result_t.packed): one 8-B word per packet holding verdict, flow hash and ACL hit ----
 * bits 0-31 flow hash | 32-36 status | 37-38 action | 39-44 flags (PPE_F_VLAN .. PPE_F_FRAG, the stateless path's
 * six) | 45-63 acl_hit + 1 (0 = -1).  Exactly the information of the three 4-B words in 8 B (13 → 9 B written per
 * packet with part8).  ppe_classify / ppe_classify_batches only, classifiers of at most PPE_PACKED_MAX_RULES rule
 * slots (the `n` of the commit). */
#define PPE_PACKED_MAX_RULES  ((1u << 19) - 1u)
#define PPE_PACKED_HASH(x)    ((uint32_t)(x))
#define PPE_PACKED_STATUS(x)  ((uint32_t)((x) >> 32) & 31u)
#define PPE_PACKED_ACTION(x)  ((uint32_t)((x) >> 37) & 3u)
#define PPE_PACKED_FLAGS(x)   ((uint32_t)((x) >> 39) & 63u)
#define PPE_PACKED_HIT(x)     ((int32_t)((uint32_t)((x) >> 45)) - 1)
#define PPE_PACKED_VERDICT(x) (PPE_PACKED_STATUS(x) | PPE_PACKED_ACTION(x) << 8 | PPE_PACKED_FLAGS(x) << 16)

/* ---- per-reason counters (sums over every batch since the last clear) ---- */
enum ppe_counter {
    PPE_C_L2_HEADERLEN_ERR = 0, PPE_C_L2_UNSUPPORT, PPE_C_L2_RX_OK,
    PPE_C_VLAN_HEADERLEN_ERR, PPE_C_VLAN_LAYER_EXCEED, PPE_C_VLAN_UNSUPPORT, PPE_C_VLAN_RX_OK,
    PPE_C_IPV4_HEADERLEN_ERR, PPE_C_IPV4_VERSION_ERR, PPE_C_IPV4_PKTLEN_ERR, PPE_C_IPV4_UNSUPPORT, PPE_C_IPV4_RX_OK,
    PPE_C_FRAG_FRAGLEN_ERR, PPE_C_FRAG_PUNT,
    PPE_C_UDP_HEADERLEN_ERR, PPE_C_UDP_PKTLEN_ERR, PPE_C_UDP_RX_OK,
    PPE_C_TCP_HEADERLEN_ERR, PPE_C_TCP_PKTLEN_ERR, PPE_C_TCP_RX_OK,
    PPE_C_ACL_DROP, PPE_C_ACL_FW,
    PPE_C_FLOW_PROC_OK, PPE_C_FLOW_PROC_FAIL, PPE_C_FLOW_TCP_NO_SYN_FIRST,
    PPE_C_OUT_FW, PPE_C_OUT_DROP, PPE_C_OUT_PUNT, PPE_C_WINDOW_PUNT, PPE_C_PKTS,
    PPE_C_FLOW_NODE_NOMEM,     /* flow table only: FlowAdd found the pool empty (decode-statistic.h:304) */
    PPE_C_RX_BYTES,            /* sum of pkt_totallen (STAT_RECV_PB_ADD, oct-rxtx.c:213)                 */
    PPE_C__COUNT /* 32 */
};

typedef struct {
    uint64_t c[32];            /* indexed by enum ppe_counter */
} ppe_counters_t;

/* ---- batch input: structure of arrays, one header window per packet ---- */
typedef struct {
    const uint8_t  *hdr;       /* n × stride bytes: the first min(len, stride) bytes of each packet            */
    const uint32_t *len;       /* n × wire length (mbuf->pkt_totallen; truncated to 16 bits like Decode())      */
    const uint64_t *ts;        /* optional n × seconds since 1970 (mbuf->timestamp); NULL → cfg->now_seconds    */
    uint32_t        n;
    uint32_t        stride;    /* a multiple of 16 from 64 to 256: 64 holds every header of a 64-B packet without
                                  VLAN / IPv4 / TCP options; 144 every byte the reference's decoders read
                                  (Ethernet 14 + VLAN 4 + IPv4 60 + TCP 60), so no WINDOW_PUNT and no
                                  PPE_TUPLE_OPT_PAST can occur                                                   */
} ppe_batch_t;

/* ---- batch output (SoA; any pointer may be NULL to skip that output) ---- */
typedef struct {
    uint32_t *verdict;         /* n × verdict word                                                            */
    uint32_t *flow_hash;       /* n × flow_hashfn(proto,sip,dip,sport,dport); 0 unless PPE_F_L4                */
    int32_t  *acl_hit;         /* n × lowest matching rule index, -1 on no match / not consulted               */
    uint32_t *fw_idx;          /* n slots: per 64-packet tile t, the FW packet indices packed at [64t, 64t+k)  */
    uint32_t *drop_idx;        /* n slots: same for DROP                                                      */
                               /* fw_idx == drop_idx selects the PARTITION layout: slots [64t, 64t+v) of tile t
                                  (v = its packet count) hold all of its packet indices, FW ascending from the
                                  front, DROP ascending at the back, PUNT ascending in between; each entry is
                                  index | action << 30 (PPE_PART_*), so no tile_cnt is needed to split them     */
    uint32_t *tile_cnt;        /* ceil(n/64) × (nfw | ndrop << 8 | npunt << 16)                                */
    uint32_t *tuple;           /* optional n × 4 words, what the reference's decoders record in the mbuf:
                                  [0] sip [1] dip (0 unless the IPv4 checks passed, decode-ipv4.c:62-63)
                                  [2] sport | dport << 16 (PPE_F_L4), or for a fragment (status FRAG /
                                      FRAG_LEN_ERR) defrag_id | frag_offset << 16 (decode-ipv4.c:107-108)
                                  [3] proto | vlan << 8 | PPE_TUPLE_WS | PPE_TUPLE_OPT_PAST | payload_len << 16
                                      (a fragment: frag_len << 16, decode-ipv4.c:109)                            */
    uint8_t  *part8;           /* optional n bytes: the PARTITION layout in compact form (with fw_idx, drop_idx
                                  and tile_cnt NULL): slot [64t + i] of tile t holds the i-th entry of the
                                  partition order above as (packet index - 64t) | action << 6 (PPE_PART8_*);
                                  1 B written per packet instead of 4 (ABI version 4)                         */
    uint64_t *packed;          /* optional n × 8 B (PPE_PACKED_*), with verdict, flow_hash and acl_hit NULL
                                  (ABI version 8)                                                             */
} ppe_result_t;

typedef struct {
    uint32_t unsupport_proto_action;  /* 0 drop (default, dp_cmd.c:37), 1 forward                            */
    uint32_t syn_check;               /* 1 (default, flow.c:26): TCP flow must start with SYN                 */
    uint64_t now_seconds;             /* timestamp used for rule time windows when batch.ts == NULL           */
} ppe_cfg_t;

typedef struct {
    uint32_t n_rules;          /* USED rules in the committed set                                          */
    uint32_t n_nodes;          /* tree nodes                                                               */
    uint32_t n_leaves;
    uint32_t n_leaf_entries;
    uint32_t max_depth;
    double   avg_depth;
    uint32_t blob_bytes;       /* device image size                                                        */
    uint32_t lds_resident;     /* 1 if the image is staged into LDS by the kernel                          */
    double   build_ms;
    uint32_t cut_bits;         /* cut-list section (image v8): sip bits | dip bits << 8; 0 with cut_entries
                                  0 = no cut lists (ABI version 6)                                            */
    uint32_t cut_entries;      /* entries of the cut lists (rules replicated into the buckets they meet)   */
} ppe_acl_stats_t;

typedef struct ppe_ctx ppe_ctx_t;

int  ppe_abi_version(void);
/* device = HIP device ordinal */
int  ppe_ctx_create(int device, ppe_ctx_t **out);
int  ppe_ctx_destroy(ppe_ctx_t *ctx);
int  ppe_ctx_device(ppe_ctx_t *ctx);

/* Build the classifier from rules[0..n) (entry i is eligible iff used == NULL || used[i] == USED) and publish it
 * for subsequent batches (double-buffered: the previous image stays valid for launches already queued).
 * n may exceed RULE_ENTRY_MAX (extended rule API, up to 1<<24).  default_action: ACL_RULE_ACTION_FW/DROP. */
int  ppe_rules_commit(ppe_ctx_t *ctx, const RCP_BLOCK_ACL_RULE_TUPLE *rules, const uint8_t *used, uint32_t n,
                      uint32_t default_action, ppe_acl_stats_t *stats);
/* The two steps of ppe_rules_commit, as the reference's commit protocol takes them (dp_cmd.c:2019-2030: build the
 * back tree, then set_running_acltree): ppe_rules_stage builds the classifier and uploads it into the back image
 * slot without publishing it (launches keep reading the running image; the upload waits only for launches that read
 * the slot it overwrites) and returns a token (> 0); ppe_rules_publish(token) makes that image the running one for
 * later launches.  A later stage replaces an unpublished one: publishing the earlier token then fails (PPE_EINVAL),
 * as does publishing a token twice.  ABI version 7. */
int  ppe_rules_stage(ppe_ctx_t *ctx, const RCP_BLOCK_ACL_RULE_TUPLE *rules, const uint8_t *used, uint32_t n,
                     uint32_t default_action, ppe_acl_stats_t *stats, uint64_t *token);
int  ppe_rules_publish(ppe_ctx_t *ctx, uint64_t token);

/* Classify one device-resident batch, enqueued on `stream` (a hipStream_t; NULL = the legacy default stream). */
int  ppe_classify(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                  void *stream);

/* Several device-resident batches (in[i] → out[i]), pipelined: consecutive batches alternate over two internal
 * streams so that one batch's launch ramp-up overlaps the previous batch's tail.  Stream-ordered like
 * ppe_classify: the batches run after the work already queued on `stream`, and work queued on `stream` after this
 * call runs after all of them.  The batches' output buffers must not overlap (two may be written at once). */
int  ppe_classify_batches(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, uint32_t nbatch,
                          const ppe_cfg_t *cfg, void *stream);

/* Host-resident batch.  When every buffer is pinned and device-mapped (hipHostMalloc, hipHostRegister, a pinned
 * torch tensor), the kernel reads and writes them across PCIe directly (zero-copy; PPE_HOST_ZEROCOPY=0 disables);
 * otherwise pipelined H2D → classify → D2H over `chunk`-packet slices on internal streams.
 * Output pointers are host pointers (NULL to skip).  Blocks until done. */
int  ppe_classify_host(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                       uint32_t chunk);

/* ppe_classify_host for a context that may have a port-scan table attached (ppe_portscan_attach).  Same arguments.
 * The outputs, the counters and the table's records after the call are those of one ppe_classify of the same batch
 * from device buffers with the same context state (StreamTcp setting included), whatever `chunk` is: the detector is
 * packet-sequential with a clock that is constant over the call, so chunks of 64 k packets taken as consecutive
 * batches give the whole batch's record grants (by first appearance), `cycle` stamps and NOMEM.
 * With the detector on (a table attached, able = 1) every chunk's pre-pass and classify launch go to one internal
 * stream in chunk order, and so do the H2D / D2H copies (measured faster than leaving them on the staging slots'
 * streams with an event each way, which PPE_HOST_ORDERED_COPY=1 at ppe_ctx_create selects).  `chunk` is rounded up to a multiple
 * of 64 and clamped to the table's max_batch rounded down to one (max_batch below 64: PPE_EINVAL); 0 = 1 << 18.
 * When every buffer is pinned and device-mapped and the batch fits max_batch, the call is one launch, as in
 * ppe_classify_host.  Without a table, or with able = 0, the call is ppe_classify_host's pipeline: equal outputs for
 * every layout that call accepts.  With attack monitors attached (ppe_attack_attach) it returns PPE_ENOTSUP before
 * touching anything.  Blocks until done. */
int  ppe_classify_host_ordered(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                               uint32_t chunk);

/* ACL-only lookup over already-decoded 5-tuples (DP_Acl_Lookup, dataplane/src/flow/flow.c:232).
 * tuple: n × 4 words {sip, dip, sport | dport << 16, proto} — the same layout as ppe_result_t.tuple;
 * macs (optional): n × 4 words {dmac bytes 0-3, dmac bytes 4-5, smac bytes 0-3, smac bytes 4-5} (little-endian);
 * ts (optional): n × seconds, else now_seconds.  hit: lowest matching rule index or -1; action: the matched rule's
 * action word or the default action. */
typedef struct {
    const uint32_t *tuple;
    const uint32_t *macs;
    const uint64_t *ts;
    uint32_t        n;
} ppe_tuples_t;
int  ppe_acl_lookup(ppe_ctx_t *ctx, const ppe_tuples_t *in, int32_t *hit, uint32_t *action, uint64_t now_seconds,
                    void *stream);                                   /* device pointers, asynchronous */
int  ppe_acl_lookup_host(ppe_ctx_t *ctx, const ppe_tuples_t *in, int32_t *hit, uint32_t *action,
                         uint64_t now_seconds);                      /* host pointers, blocking */

/* Memory helpers for C integrators (device / pinned host buffers on the context's device). */
void *ppe_dev_alloc(ppe_ctx_t *ctx, size_t bytes);
void  ppe_dev_free(ppe_ctx_t *ctx, void *p);
void *ppe_host_alloc(ppe_ctx_t *ctx, size_t bytes);   /* pinned */
void  ppe_host_free(ppe_ctx_t *ctx, void *p);
int   ppe_memcpy_h2d(ppe_ctx_t *ctx, void *dst, const void *src, size_t bytes);
int   ppe_memcpy_d2h(ppe_ctx_t *ctx, void *dst, const void *src, size_t bytes);
int   ppe_memset_d(ppe_ctx_t *ctx, void *dst, int value, size_t bytes);
int   ppe_sync(ppe_ctx_t *ctx);

/* Counters: per-workgroup slots in device memory, reduced on read.  Synchronises the device. */
int  ppe_counters_read(ppe_ctx_t *ctx, ppe_counters_t *out);
int  ppe_counters_clear(ppe_ctx_t *ctx);

/* ---- StreamTcp's first-packet verdict on the stateless classify path (dataplane/src/plugin/stream-tcp/stream-tcp.c) ----
 * The reference runs every TCP packet the ACL forwarded through StreamTcp (flow.c:311-320); for a packet without a
 * session the decision is StreamTcpPacketStateNone (stream-tcp.c:237-441), a function of th_flags and these words.
 * The stateless path treats every packet as the first of its flow, so with track = 1 ppe_classify,
 * ppe_classify_batches and ppe_classify_host apply that decision to every TCP packet with status PPE_ST_ACL_FW:
 *   RST → PPE_ST_STREAM_RST_NO_SESSION; else FIN → PPE_ST_STREAM_FIN_NO_SESSION; else SYN|ACK →
 *   PPE_ST_STREAM_MIDSTREAM_ONESIDE_OFF unless midstream or async_oneside; else SYN → forward; else ACK →
 *   PPE_ST_STREAM_MIDSTREAM_OFF (midstream 0); anything else forwards (stream-tcp.c:434-437).
 * A stream drop keeps acl_hit, PPE_F_ACL, the flow hash, the tuple and every flag, and counts in ppe_counters_t what
 * the reference has counted by then: ACL_FW (flow.c:240), FLOW_PROC_OK (flow.c:309), OUT_DROP; not FLOW_PROC_FAIL.
 * A new context starts at {0,0,0,0} (tracking off: results and counters exactly as without this interface; the
 * reference itself starts with tracking on, stream-tcp.c:16,20-21).  ppe_stream_tcp_set(ctx, NULL) selects the
 * reference's defaults {1,0,0,1}; a word above 1 is PPE_EINVAL.  reasm only feeds ppe_format_tcpstream_stat.  The
 * setting travels by value with each launch: it applies to launches enqueued after the call, no synchronisation.
 * Not supported (PPE_ENOTSUP): track && midstream && !syn_check on the stateless calls (an ACK-only packet would
 * enter segment reassembly, stream-tcp.c:371-432), and ppe_classify_flow with track unless the session state machine
 * is attached to the flow table (ppe_flow_stream_attach, below: later packets of a flow need it, stream-tcp.c:3005-3140;
 * with it attached reasm also selects, and must be 0); the flow table stays usable. */
typedef struct { uint32_t track, midstream, async_oneside, reasm; } ppe_stream_tcp_cfg_t;
int  ppe_stream_tcp_set(ppe_ctx_t *ctx, const ppe_stream_tcp_cfg_t *cfg);
int  ppe_stream_tcp_get(ppe_ctx_t *ctx, ppe_stream_tcp_cfg_t *cfg);

/* tcpstreamtrackstat counters this path produces (STREAM_* macros, stream-tcp.c:2989-3003 counted for every tracked
 * packet before the decision, then one per drop reason); SESSION_NO_MEM has no stateless meaning and stays 0 */
enum ppe_stream_counter { PPE_SC_SYN_ACK_COUNT, PPE_SC_SYN_COUNT, PPE_SC_RST_COUNT, PPE_SC_RST_BUT_NO_SESSION,
  PPE_SC_FIN_BUT_NO_SESSION, PPE_SC_MIDSTREAM_OR_ONESIDE_DISABLE, PPE_SC_MIDSTREAM_DISABLE, PPE_SC_PKT_BROKEN_ACK,
  PPE_SC__COUNT };
typedef struct { uint64_t c[16]; } ppe_stream_counters_t;   /* indexed by enum ppe_stream_counter; the rest 0 */
int  ppe_stream_counters_read(ppe_ctx_t *ctx, ppe_stream_counters_t *out);   /* synchronises, like ppe_counters_read */
int  ppe_stream_counters_clear(ppe_ctx_t *ctx);                              /* dp_clear_tcpstream_stat, dp_cmd.c:156 */
/* `show tcpstream statistic` text (dp_show_tcpstream_stat, dp_cmd.c:174-842: same lines, order and labels; the
 * enable / disable lines from cfg->track and cfg->reasm, NULL cfg = both disabled; counters this engine does not
 * produce print 0).  snprintf semantics, like ppe_format_pkt_stat. */
int  ppe_format_tcpstream_stat(const ppe_stream_counters_t *c, const ppe_stream_tcp_cfg_t *cfg, char *buf, size_t cap);

/* Kernel timing with HIP events recorded around each ppe_classify launch on its stream. */
int  ppe_timing_enable(ppe_ctx_t *ctx, int on);
/* Synchronises, then returns the sum of launch durations (ms) and the launch count since the last reset. */
int  ppe_timing_read(ppe_ctx_t *ctx, double *total_ms, uint32_t *launches, int reset);

/* Copy the current device classifier image to host (for tests / tools).  words may be NULL to query size. */
int  ppe_acl_image(ppe_ctx_t *ctx, uint32_t *words, uint32_t *n_words);

/* Launch tuning of the classify kernel for this context.  Defaults come from the fastest measured variant (and the
 * PPE_BLOCK / PPE_BLOCKS_PER_CU / PPE_PIPELINE / PPE_LDS_IMG environment variables); 0 = automatic. */
typedef struct {
    uint32_t block;          /* workgroup size 256, 512 or 1024; 0 = chosen per classifier image   */
    uint32_t blocks_per_cu;  /* workgroups per CU (<= 32); 0 = resident count from the occupancy API */
    uint32_t pipeline;       /* tile fetch / walk: 0 auto (4 when the image's tree fits in LDS, else 5
                                when it has cut lists, else 3), 1 first tile loaded at the loop top,
                                4 first tile requested before the image staging, 3 four tiles per
                                wave loaded, decoded and walked together through the 2-level blocks
                                (one 1024-thread workgroup per CU), 5 the cut lists (image v7: one
                                tile per wave, bucket groups in LDS, list entries from L2; an image
                                without cut lists takes the automatic choice); others PPE_EINVAL   */
    uint32_t lds_image;      /* 1 = stage the image (or its top) in LDS, 0 = read it from global   */
    uint32_t batches_per_launch;  /* ppe_classify_batches: batches one launch takes (<= 4096); 0 = all
                                     of a call's batches in ONE persistent launch (descriptor ring)  */
} ppe_tuning_t;
int  ppe_set_tuning(ppe_ctx_t *ctx, const ppe_tuning_t *t);
int  ppe_get_tuning(ppe_ctx_t *ctx, ppe_tuning_t *t);

/* Launch geometry in use (for profiling notes).  variant = image mode (0 global, 1 LDS, 2 split) | fetch << 4
 * (fetch 0 first tile at the loop top, 1 first tile requested before the image staging, 3 four tiles per wave,
 * 5 cut lists). */
int  ppe_launch_info(ppe_ctx_t *ctx, uint32_t *grid, uint32_t *block, uint32_t *lds_bytes, uint32_t *variant);


/* ---- Stateful flow table (dataplane/src/flow/flow.c) ----
 * One table per context (the reference keeps one per core, flow_table[LOCAL_CPU_ID]; across GPUs, shard packets by
 * flow hash so each flow lives on one device).  ppe_classify_flow() runs the reference's FlowHandlePacket for a whole
 * batch with exactly the sequential semantics of one core processing the batch in index order:
 *   - a packet whose flow exists (FlowFind: 5-tuple match in either direction, flow.c:81-115) is forwarded without
 *     an ACL lookup, counted ACL_FW / FLOW_PROC_OK, and updates the flow's per-direction packet / byte counters
 *     (FlowUpdate, flow.c:163-178, bytes = pkt_totallen) and last-seen time (FLOW_UPDATE_TIMESTAMP = cfg->now_seconds);
 *   - otherwise syn_check and the ACL decide as in the stateless path; an ACL FW creates the flow (FlowAdd, oriented
 *     as that packet), or fails with PPE_ST_FLOW_NOMEM when `capacity` flows are live (flow.c:124-129);
 *   - later packets of the same batch see flows created by earlier ones (in index order).
 * acl_hit is -1 and PPE_F_ACL clear for packets that found their flow.  Aging (FlowTimeOut / FlowAgeTimeoutCB, flow.c:391-467) is
 * explicit: ppe_flow_age() removes flows idle for more than `timeout_seconds` (reference: FLOW_MAX_TIMEOUT = 20 s).
 * Batches go through one stream in order; out->verdict is required; n <= max_batch. */
typedef struct {
    uint32_t sip, dip;            /* flow_item_t.ipv4 of the creating packet (flow.h:57)                        */
    uint16_t sport, dport;
    uint8_t  protocol, pad[3];
    uint32_t flowflags;           /* FLOW_FLAG_* (always 0: nothing sets PERSISTENT in the reference)            */
    uint32_t slot;                /* device table slot (diagnostic)                                              */
    uint64_t pktcnts2d, pktcntd2s, bytecnts2d, bytecntd2s;   /* flow.h:66-69                                       */
    uint64_t last_seen;           /* `cycle`: cfg->now_seconds of the last packet of the flow                    */
} ppe_flow_entry_t;

typedef struct {
    uint64_t live;                /* flows in the table                                                          */
    uint64_t new_flow, del_flow;  /* FlowAdd / aging totals since create or ppe_flow_clear_stat (dp_cmd.c:2327)  */
    uint32_t capacity;            /* flow pool size (reference MEM_POOL_FLOW_NODE_NUM = 100000)                  */
    uint32_t max_batch;
    uint32_t slots;               /* open-addressing slots (power of two >= 2 x (capacity + max_batch))          */
    uint32_t tombstones;          /* deleted slots not yet reclaimed by a rehash                                 */
    uint32_t rehashes;
    uint32_t pad;
} ppe_flow_info_t;

/* FlowInit (flow.c:471-516): create / replace the context's table.  capacity 0 = 100000, max_batch 0 = 1<<20. */
int  ppe_flow_create(ppe_ctx_t *ctx, uint32_t capacity, uint32_t max_batch);
int  ppe_flow_destroy(ppe_ctx_t *ctx);                                /* FlowRelease (flow.c:519-530) */
/* FlowHandlePacket for a device-resident batch (same buffers as ppe_classify), stream-ordered on `stream`.
 * A batch is two launches (classify, then finalize + counter update); a small batch (at most PPE_FLOW_SMALL_CUTOFF
 * packets, csrc/ppe_internal.h) is one launch of one workgroup that runs both phases, with the same results and the
 * same table (PPE_FLOW_SMALL=0 in the environment at ppe_flow_create: always two; with monitors flow-attached: always
 * two).  The two shapes interleave freely on one table.  If the second of two launches cannot be launched, the call
 * returns PPE_EIO and the table is unusable from then on: every later ppe_classify_flow / ppe_flow_age / _info /
 * _clear_stat / _dump returns PPE_EIO at once, until ppe_flow_destroy (or a new ppe_flow_create). */
int  ppe_classify_flow(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                       void *stream);
/* FlowHandlePacket for a host-resident batch (same buffers as ppe_classify_host).  Blocks until done.
 * The per-packet outputs only: verdict (required), flow_hash, acl_hit, tuple.  A compacted list (fw_idx, drop_idx,
 * tile_cnt, part8) or `packed` returns PPE_EINVAL before anything is touched (the post kernel has no index base for a
 * chunk; lists across chunks are not built).
 * The batch runs as consecutive ppe_classify_flow batches of `chunk` packets; H2D, both launches and D2H of every chunk
 * go to one internal stream in chunk order (the stream of ppe_classify_host_ordered).  The flow path is exactly
 * sequential and cfg->now_seconds is constant over the call, so the outputs, the counters and the whole table after
 * the call are those of one core running the batch in index order, whatever `chunk` is: equal to one
 * ppe_classify_flow of the same packets from device buffers.  `chunk` is rounded up to a multiple of 64 and clamped
 * to the table's max_batch rounded down to one (max_batch below 64: PPE_EINVAL); 0 = min(1 << 18, that).
 * When every buffer is pinned and device-mapped, n <= max_batch and PPE_HOST_ZEROCOPY is not 0, the kernels read and
 * write the host buffers directly: one flow batch, no staging copy.
 * PPE_ENOTSUP before touching anything: wherever ppe_classify_flow refuses (stream tracking on, a port-scan table
 * attached with ppe_portscan_attach, an object attached with ppe_attack_attach), and with an object attached with
 * ppe_flow_attack_attach (its per-batch port array does not map onto chunks).  A broken table: PPE_EIO, as
 * ppe_classify_flow.
 * With a port-scan table flow-attached and its detector on (ppe_flow_portscan_attach, able 1) the chunk is clamped to a
 * multiple of 64 of at most ppe_flow_portscan_max() as well, batch.ts is taken per chunk, and the zero-copy form
 * applies when n <= ppe_flow_portscan_max(); the result is still one core's run of the whole batch, whatever the chunk.
 * Flow batches submitted earlier on other streams must have completed (the internal stream does not wait for them). */
int  ppe_classify_flow_host(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                            uint32_t chunk);
/* ppe_classify_flow_host plus a host array of in->n input-port bytes for the flow-attached attack monitors
 * (ppe_flow_attack_attach), which ppe_classify_flow_host refuses.  ports NULL: port 0 for every packet; the kernels use
 * port & 3; the sticky device table of ppe_attack_ports is not read by this call.
 *   - Nothing flow-attached (or only a port-scan table): byte for byte ppe_classify_flow_host, in outputs, counters,
 *     table and launch kinds; ports is ignored.
 *   - Monitors flow-attached: every chunk runs ppe_flow_attack_attach's semantics with its slice of ports; the clock is
 *     ppe_attack_clock / _tick's value at the call (no tick inside a call).  The result is one core's run of the whole
 *     batch in index order, whatever `chunk` is: the flow path is exactly sequential, and between two ticks a monitor's
 *     verdict depends only on the packet and the interval's starting state.  A chunk of at most 256 packets
 *     (PPE_FLOW_SMALL_ATK_CUTOFF, measured) runs in one launch (ppe_flow_launch_info kind 4; not under
 *     PPE_FLOW_SMALL=0), a larger one in two (kind 0).  ppe_classify_flow itself never takes kind 4: with monitors attached and no
 *     detector it reports (0, 2) at every size.
 *   - Monitors and a port-scan table both flow-attached, its detector on: with ppe_flow_combine on, chunks of at most
 *     ppe_flow_portscan_max() packets, each through the combined kernel (kind 3), batch.ts taken per chunk; with the
 *     switch off PPE_ENOTSUP before anything is touched, as ppe_classify_flow.
 * Every other refusal of ppe_classify_flow_host is kept (stream tracking, a stateless-attached table or object, lists
 * or packed, max_batch below one tile).  A chunk's port bytes are copied on the same internal stream ahead of its
 * launch; the zero-copy form applies only when ports is NULL or itself pinned and device-mapped, otherwise the staged
 * path runs. */
int ppe_classify_flow_host_ports(ppe_ctx_t *ctx, const ppe_batch_t *in, const ppe_result_t *out,
                                 const ppe_cfg_t *cfg, uint32_t chunk, const uint8_t *ports);
/* What the last flow batch of the context's table took: *kind 1 and *launches 1 (the one-launch kernel), 2 and 1 (the
 * one-launch kernel with the port-scan detector inside, ppe_flow_portscan_attach), 3 and 1 (that kernel with the
 * flow-attached attack monitors in it as well, ppe_flow_combine), 4 and 1 (the one-launch kernel with the
 * flow-attached monitors in it: chunks of ppe_classify_flow_host_ports only), or 0 and 2; 0 and 0 before the first
 * batch; 5 and 1: the one-launch kernel with the TCP session machine behind it (ppe_flow_stream_attach); 6 and 1:
 * that kernel with the flow-attached monitors in it as well (ppe_flow_stream_monitors); 7 and 1: the one-launch kernel
 * with the port-scan detector inside and the TCP session machine behind it (ppe_flow_stream_portscan); 8 and 1: that
 * kernel with the flow-attached monitors in it as well.  NULL arguments: PPE_EINVAL. */
int  ppe_flow_launch_info(ppe_ctx_t *ctx, uint32_t *kind, uint32_t *launches);
/* FlowAgeTimeoutCB: delete flows with now > last_seen && now - last_seen > timeout_seconds; *deleted = count
 * (may be NULL).  Synchronises. */
int  ppe_flow_age(ppe_ctx_t *ctx, uint64_t now_seconds, uint64_t timeout_seconds, uint64_t *deleted);
int  ppe_flow_info(ppe_ctx_t *ctx, ppe_flow_info_t *info);         /* dp_show_flow_stat (dp_cmd.c:2346); syncs */
int  ppe_flow_clear_stat(ppe_ctx_t *ctx);                           /* dp_clear_flow_stat (dp_cmd.c:2327) */
/* Copy up to `max` live flows to host (table order); *n = live flows.  Synchronises. */
int  ppe_flow_dump(ppe_ctx_t *ctx, ppe_flow_entry_t *entries, uint32_t max, uint32_t *n);

/* ---- StreamTcp's session state machine on the flow-table path (dataplane/src/plugin/stream-tcp/stream-tcp.c) ----
 * The reference runs every TCP packet that has a flow through StreamTcpPacket (flow.c:311-320) and drops what it
 * rejects.  ppe_flow_stream_attach(ctx, 1) builds that behind the flow table: one 64-B session record per flow slot,
 * stepped in packet order.  It runs when a flow table exists, the switch is on, and ppe_stream_tcp_set holds
 * {track 1, midstream 0, async_oneside 0, reasm 0}: the reference's defaults with segment reassembly switched off
 * (stream_tcp_reasm_enable, dp_cmd.c:2100), under which StreamTcpReassembleHandleSegment returns OK at once
 * (stream-tcp-reassemble.c:460-464), no packet is cached and StreamTcp is OK or ERR.  With the switch off (a new
 * context) every call, refusal, output and counter is what it was.
 *   Packets: every TCP packet that ends FlowHandlePacket with a flow (status PPE_ST_ACL_FW with PPE_F_FLOW: found, or
 *   the creator).  UDP, packets without a flow and decode drops are untouched, and the flow table is exactly what the
 *   plain path leaves: FlowAdd, FlowUpdate, last-seen and the counters come before StreamTcp (flow.c:304-311).
 *   Order: one core running the batch in index order; sessions of different flows do not interact.
 *   Direction: PPE_F_TOCLIENT set is PKT_IS_TOCLIENT, clear PKT_IS_TOSERVER.  payload_len, TCP_GET_SEQ / _ACK /
 *   _WINDOW and tcpvars.ws / TCP_GET_WSCALE are read from the TCP header as the reference's macros read them.
 *   A dropped packet keeps flow hash, tuple, acl_hit and every flag; its action becomes DROP and it moves to the drop
 *   list / partition.  StreamTcpPacketStateNone's four reasons are statuses 20-23, every other reason is
 *   PPE_ST_STREAM_TRACK_DROP with the reason in the flags.  ppe_counters_t counts FLOW_PROC_OK, ACL_FW and OUT_DROP.
 *   The engine's definition where the reference leaves the value open (StreamTcpNewSession sets state and nothing
 *   else, stream-tcp-session.c:22-33, and client.window is read at stream-tcp.c:835 before any branch wrote it): a
 *   session record is all zero when its flow is created (a PPE_F_NEWFLOW packet zeroes its slot's record before its
 *   step), and a found flow without a session has an all-zero record.  Attaching zeroes every record, and so does
 *   ppe_stream_tcp_set changing track 0 -> 1 while attached: flows alive then have no session (ssn == NULL).  A
 *   rehash moves the records with their flows.  Not kept: ra_app_base_seq, ra_raw_base_seq, last_ts, last_pkt_ts,
 *   os_policy, the segment lists.
 * Refused before anything is touched: attached with track 1 and any of reasm, midstream, async_oneside 1
 * (PPE_ENOTSUP); a port-scan table flow-attached at the same time unless ppe_flow_stream_portscan is on, or monitors
 * flow-attached unless ppe_flow_stream_monitors is on (PPE_ENOTSUP); a device batch of more
 * than ppe_flow_stream_max() packets (PPE_ENOTSUP; ppe_classify_flow_host takes host batches of any size in chunks
 * of at most that); a header stride under 144 B (PPE_EINVAL: neither PPE_ST_WINDOW_PUNT nor PPE_TUPLE_OPT_PAST may
 * stand between a SYN and its window scale); attach without a flow table (PPE_EINVAL).  Attached with track 0 the
 * context runs the plain kernels.  One launch per batch (ppe_flow_launch_info kind 5). */
int  ppe_flow_stream_attach(ppe_ctx_t *ctx, uint32_t on);
uint32_t ppe_flow_stream_max(void);
#define PPE_FLOW_STREAM_MIN_STRIDE 144u
/* a side of a session (TcpStream, stream-tcp-private.h:118-144) and a live TCP flow's key with its session record
 * (TcpSession, :147-153; state 0 = TCP_NONE .. 11 = TCP_CLOSED) */
typedef struct { uint32_t isn, next_seq, last_ack, next_win, window; uint16_t flags; uint8_t wscale, pad; } ppe_stream_side_t;
typedef struct {
    uint32_t sip, dip;
    uint16_t sport, dport;
    uint32_t slot;                /* device table slot (diagnostic) */
    uint16_t flags;               /* STREAMTCP_FLAG_* */
    uint8_t  state, pad;          /* pad: the flow's input port, flow_item_t.input_port (ppe_flow_stream_monitors; else 0) */
    ppe_stream_side_t client, server;
} ppe_flow_stream_entry_t;
/* Copy up to `max` live TCP flows with their sessions to host (table order); *n = live TCP flows.  Synchronises. */
int  ppe_flow_stream_dump(ppe_ctx_t *ctx, ppe_flow_stream_entry_t *entries, uint32_t max, uint32_t *n);
/* ---- Monitors flow-attached and sessions attached on one batch: syncount_accum as the gauge of half-open connections ----
 * 0 (a new context): as before, the two together are refused.  1: with sessions attached, ppe_stream_tcp_set holding
 * {1,0,0,0}, an object attached with ppe_flow_attack_attach and no port-scan table flow-attached, ppe_classify_flow takes
 * a batch of 1 <= n <= ppe_flow_stream_max() packets (stride >= PPE_FLOW_STREAM_MIN_STRIDE) in one launch
 * (ppe_flow_launch_info kind 6), exactly one core running the batch in index order: the monitors first, for every packet,
 * as under ppe_flow_attack_attach alone (a packet they drop reaches neither the table nor its session: a SYN|ACK the
 * SYN-flood monitor drops leaves its session in SYN_SENT); the survivors take ppe_flow_stream_attach's path unchanged.
 * on > 1: PPE_EINVAL.  The context's, like ppe_flow_combine: ppe_flow_destroy leaves it; no synchronisation.
 *   syncount_accum: +1 on the packet's port for a TCP SYN that ends with PPE_F_NEWFLOW, as under ppe_flow_attack_attach
 *   (FlowAdd runs before StreamTcp: whatever the session's verdict); -1 on the port of the packet whose step takes its
 *   session from SYN_RECV to ESTABLISHED (DP_Attack_SynCountFins, stream-tcp.c:608 and :660, on m->input_port: that
 *   packet's port, not the flow's); -1 on the flow's port for every TCP flow ppe_flow_age deletes while its session is
 *   in the handshake (StreamTcp_Flow_ResRelease, stream-tcp-session.c:61-77: state not NONE and at most SYN_RECV), once
 *   per deleted flow, visible to the next ppe_attack_info and folded by the next ppe_attack_tick, whatever track is.
 *   The flow's port is its creating packet's (flow_item_t.input_port, flow.c:139; a flow created while no monitors were
 *   flow-attached, or by the kernel without them: port 0); ppe_flow_stream_dump reports it in `pad`.
 *   The arithmetic is the reference's cvmx_atomic_add64 on a uint64_t, modulo 2^64, and so is this: a port that
 *   establishes more than it created in an interval (a handshake that completes on another port than its SYN's, or a
 *   session reused from CLOSED, which takes a second -1 with no +1) shows syncount_accum: -1 in ppe_format_attack_stat,
 *   its syncount is 2^64 - 1 after the tick, and with td.drop_pack 1 every SYN on it is then PPE_ST_ATTACK_SYNCOUNT
 *   until the next tick.  That is the reference's behaviour, reproduced.
 * ppe_classify_flow_host_ports runs host batches of any size under the same conditions (chunks of at most
 * ppe_flow_stream_max(), each one launch with its slice of `ports`); ppe_classify_flow_host keeps refusing monitors
 * flow-attached.  Still refused before anything is touched: the switch off, a port-scan table flow-attached as well
 * (whatever its able; ppe_flow_stream_portscan, below, lifts this), a larger device batch, reasm / midstream /
 * async_oneside 1 (PPE_ENOTSUP); a stride under 144 B (PPE_EINVAL).  With the switch on but only one of the two attached, or track 0, nothing changes. */
int  ppe_flow_stream_monitors(ppe_ctx_t *ctx, uint32_t on);
/* ---- A port-scan table flow-attached and sessions attached on one batch: the reference's default pipeline ----
 * Decode -> attack monitors -> FlowHandlePacket -> FlowFind | miss -> syn_check -> PortScan_Detect -> DP_Acl_Lookup ->
 * FlowAdd -> FlowUpdate -> StreamTcp (flow.c:196-243, :271-320), with portscan_able 1 and stream_tcp_track_enable 1.
 * 0 (a new context): as before, the two together are refused, and every call, refusal, kernel, launch kind and result
 * is what it was.  on > 1: PPE_EINVAL.  The context's, like ppe_flow_combine and ppe_flow_stream_monitors:
 * ppe_flow_destroy leaves it; no synchronisation.
 * 1, with sessions attached, ppe_stream_tcp_set holding {1,0,0,0} and a table attached with ppe_flow_portscan_attach whose
 * able is 1: ppe_classify_flow takes a batch of 1 <= n <= min(ppe_flow_portscan_max(), ppe_flow_stream_max()) packets
 * (stride >= PPE_FLOW_STREAM_MIN_STRIDE) in one launch.  No monitors flow-attached: ppe_flow_launch_info kind 7.  Monitors
 * flow-attached as well: ppe_flow_combine and ppe_flow_stream_monitors must both be 1 (each pair has been opted into), and
 * the kind is 8; with either off the call is refused as before.  Exactly one core running the batch in index order:
 *   1. the monitors, if attached, as under ppe_flow_combine (1): a packet they drop reaches neither table nor the
 *      detector nor its session;
 *   2. the survivors take ppe_flow_portscan_attach's path unchanged: a packet that finds its flow is never at the
 *      detector; the rest take syn_check, PortScan_Detect, then PPE_ST_PORTSCAN_DROP, or the ACL and FlowAdd or
 *      PPE_ST_FLOW_NOMEM;
 *   3. every packet that ends PPE_ST_ACL_FW with PPE_F_FLOW | PPE_F_TCP steps its flow's session exactly as under
 *      ppe_flow_stream_attach, a PPE_F_NEWFLOW packet from the zero record.  A packet that ends PPE_ST_PORTSCAN_DROP,
 *      PPE_ST_FLOW_TCP_NO_SYN_FIRST, PPE_ST_ACL_DROP or PPE_ST_FLOW_NOMEM has no flow: it takes no step and counts in no
 *      stream counter.  A stream drop (status 20-23, or 29 with the reason bits; action DROP; OUT_FW handed to OUT_DROP)
 *      keeps the flow, the detector's record and every flag: StreamTcp runs behind FlowAdd and FlowUpdate and its
 *      verdict feeds nothing back (flow.c:304-319);
 *   4. kind 8: syncount_accum takes +1 on the packet's port for a TCP SYN that ends with PPE_F_NEWFLOW and -1 on the
 *      completing packet's port for SYN_RECV -> ESTABLISHED, as under ppe_flow_stream_monitors; session record word 13 is
 *      the creating packet's port, and ppe_flow_age's release pass runs under its condition, so a scan's half-open flows
 *      give their +1 back when they age out.  Kind 7 stores 0 there.
 * 1 with able != 1: the detector is off, so the batch runs as if no table were flow-attached (kinds 5 / 6, their results
 * byte for byte).  1 with only the sessions or only the table attached, or track 0: nothing changes.
 * ppe_classify_flow_host runs host batches of any size as kind 7 per chunk (a multiple of 64, at most the smaller of the
 * two maxima and of both tables' max_batch; `ts` per chunk), ppe_classify_flow_host_ports as kind 8 per chunk with its
 * slice of `ports`: one core's run of the whole batch whatever the chunk (only the flow table's tombstone count may
 * differ).  Refused before anything is touched: a larger device batch, reasm / midstream / async_oneside 1
 * (PPE_ENOTSUP); a stride under 144 B, n above the port-scan table's max_batch (PPE_EINVAL). */
int  ppe_flow_stream_portscan(ppe_ctx_t *ctx, uint32_t on);
/* struct tcpstream_track_stat (decode-statistic.h:118-179), every field in the reference's order; the session path
 * counts here (the stateless path keeps feeding ppe_stream_counters_t) */
enum ppe_stream_track_counter {
    PPE_STC_SYN_ACK_COUNT, PPE_STC_SYN_COUNT, PPE_STC_RST_COUNT, PPE_STC_RST_BUT_NO_SESSION,
    PPE_STC_FIN_BUT_NO_SESSION, PPE_STC_MIDSTREAM_OR_ONESIDE_DISABLE, PPE_STC_MIDSTREAM_DISABLE,
    PPE_STC_ONESIDE_DISABLE, PPE_STC_SESSION_NO_MEM, PPE_STC_FIN_INVALID_ACK, PPE_STC_FIN_OUT_OF_WINDOW,
    PPE_STC_SESSION_PARAM_ERR, PPE_STC_WHS3_SYNACK_TOSERVER_SYN_RECV, PPE_STC_WHS3_SYNACK_SEQ_MISMATCH,
    PPE_STC_WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK, PPE_STC_WHS3_SYN_TOCLIENT_ON_SYN_RECV,
    PPE_STC_WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV, PPE_STC_WHS3_SYNACK_IN_WRONG_DIRECTION,
    PPE_STC_WHS3_ACK_IN_WRONG_DIR, PPE_STC_WHS3_RIGHT_SEQ_WRONG_ACK_EVASION, PPE_STC_WHS3_WRONG_SEQ_WRONG_ACK,
    PPE_STC_WHS3_ASYNC_WRONG_SEQ, PPE_STC_WHS3_SYNACK_WITH_WRONG_ACK, PPE_STC_WHS4_WRONG_SEQ,
    PPE_STC_WHS4_INVALID_ACK, PPE_STC_WHS4_SYNACK_WITH_WRONG_ACK, PPE_STC_WHS4_SYNACK_WITH_WRONG_SYN,
    PPE_STC_EST_INVALID_ACK, PPE_STC_EST_PKT_BEFORE_LAST_ACK, PPE_STC_EST_PACKET_OUT_OF_WINDOW,
    PPE_STC_EST_SYNACK_RESEND, PPE_STC_EST_SYNACK_TOSERVER, PPE_STC_EST_SYNACK_RESEND_WITH_DIFFERENT_ACK,
    PPE_STC_EST_SYNACK_RESEND_WITH_DIFF_SEQ, PPE_STC_EST_SYN_TOCLIENT, PPE_STC_EST_SYN_RESEND_DIFF_SEQ,
    PPE_STC_EST_SYN_RESEND, PPE_STC_PKT_RETRANSMISSION, PPE_STC_FIN2_FIN_WRONG_SEQ, PPE_STC_FIN2_INVALID_ACK,
    PPE_STC_FIN2_ACK_WRONG_SEQ, PPE_STC_FIN1_FIN_WRONG_SEQ, PPE_STC_FIN1_INVALID_ACK, PPE_STC_FIN1_ACK_WRONG_SEQ,
    PPE_STC_SHUTDOWN_SYN_RESEND, PPE_STC_CLOSEWAIT_FIN_OUT_OF_WINDOW, PPE_STC_CLOSING_ACK_WRONG_SEQ,
    PPE_STC_CLOSEWAIT_INVALID_ACK, PPE_STC_CLOSING_INVALID_ACK, PPE_STC_CLOSEWAIT_PKT_BEFORE_LAST_ACK,
    PPE_STC_CLOSEWAIT_ACK_OUT_OF_WINDOW, PPE_STC_LASTACK_ACK_WRONG_SEQ, PPE_STC_LASTACK_INVALID_ACK,
    PPE_STC_TIMEWAIT_ACK_WRONG_SEQ, PPE_STC_TIMEWAIT_INVALID_ACK, PPE_STC_PKT_INVALID_ACK,
    PPE_STC_PKT_BAD_WINDOW_UPDATE, PPE_STC_PKT_BROKEN_ACK, PPE_STC__COUNT /* 58 */
};
typedef struct { uint64_t c[64]; } ppe_stream_track_counters_t;   /* indexed by the enum above; words 58-63 zero */
int  ppe_stream_track_counters_read(ppe_ctx_t *ctx, ppe_stream_track_counters_t *out);   /* synchronises */
int  ppe_stream_track_counters_clear(ppe_ctx_t *ctx);
/* `show tcpstream statistic` text (dp_show_tcpstream_stat, dp_cmd.c:174-842) from the 64-word block: every track line
 * from its own counter, the reassembly lines 0.  Returns the length written, or -needed when cap is too small. */
int  ppe_format_tcpstream_stat_ex(const ppe_stream_track_counters_t *c, const ppe_stream_tcp_cfg_t *cfg, char *buf,
                                  size_t cap);

/* ---- Flow-hash steering across GPUs (the stateful path shards by flow, like Octeon's PIP tag
 * steering of a flow to one core, dataplane/src/platform/oct-init.c:139-151) ----
 * ppe_steer_partition: from a stateless ppe_classify of the batch (verdict + flow_hash), each packet's owner GPU is
 * flow_hash % world if it reaches the flow table (PPE_F_L4), else `rank` (its stateless verdict is final anyway).
 * perm[n] = packet indices grouped by owner, ascending within each owner; counts[world] = packets per owner.
 * ppe_gather_rows: dst[i] = src[perm[i]]; ppe_scatter_rows: dst[perm[i]] = src[i] (rows of row_bytes, a multiple of
 * 4, <= 256).  All device pointers, stream-ordered.  world <= 16.  The exchange itself is an all-to-all of the
 * gathered windows (RCCL over xGMI), then ppe_classify_flow on the received packets and the reverse all-to-all of
 * their verdicts: packet-process-engine_amd/ppe/dist.py steered_classify_flow. */
int  ppe_steer_partition(ppe_ctx_t *ctx, const uint32_t *verdict, const uint32_t *flow_hash, uint32_t n,
                         uint32_t world, uint32_t rank, uint32_t *perm, uint32_t *counts, void *stream);
int  ppe_gather_rows(ppe_ctx_t *ctx, const void *src, uint32_t row_bytes, const uint32_t *perm, uint32_t n,
                     void *dst, void *stream);
int  ppe_scatter_rows(ppe_ctx_t *ctx, const void *src, uint32_t row_bytes, const uint32_t *perm, uint32_t n,
                      void *dst, void *stream);

/* Operator text of the reference's `show` commands, from counters / flow info read with ppe_counters_read /
 * ppe_flow_info: dp_show_pkt_stat (dataplane/src/common/dp_cmd.c:844-1818; same sections, names and order; the
 * reference's SELF_TEST build (flow.c:21) never counts output_*, and the I/O, ARP/ICMP/OSPF, TX and other attack
 * counters have no source on this path: those lines print 0) and dp_show_flow_stat (dp_cmd.c:2346-2392); the
 * reassembly lines come from ppe_defrag_info (ppe_format_*_ex, declared with the reassembly API below).
 * snprintf semantics: returns the full length, writes at most cap bytes including the NUL. */


/* ---- IPv4 reassembly (dataplane/src/decode/decode-defrag.c) ----
 * ppe_classify PUNTs fragments (PPE_ST_FRAG).  ppe_defrag runs the reference's Defrag (decode-defrag.c:449-487) for
 * a batch of them, with exactly the sequential semantics of one core handling the fragments in index order:
 *   FragFind / fcb_create on (sip, dip, ip_id) (decode-defrag.c:115-146, 71-97; at most fcb_max FCBs, STAT_FRAG_FCB_FULL),
 *   PACKET_HW2SW into a 2 KB buffer (mbuf.c:117-156: pkt_totallen > frag_buf_bytes drops, STAT_FRAG_HW2SW_ERR),
 *   the DELETE / cache_max checks of Frag_defrag_begin (decode-defrag.c:412-446) and Frag_defrag_process
 *   (decode-defrag.c:292-406) — ordered fragment chain, overlap ("teardrop") and last-fragment checks, including the
 *   reference's chain scan that compares frag_len (not frag_offset) with the new offset (decode-defrag.c:344-349);
 *   on completion Frag_defrag_reasm (decode-defrag.c:222-289): the head fragment's whole frame followed by every
 *   later fragment's last frag_len bytes, ip_len = ihl*4 + total, ip_off = 0, header checksum recomputed (ICMP: the
 *   head frame only, ip_off = 0).  A datagram whose buffer (total + L2 + ihl*4) exceeds reasm_buf_bytes fails as
 *   STAT_FRAG_SETUP_ERR (MEM_8K_ALLOC, decode-defrag.c:173-183) and its fragments stay cached.
 * Reassembled datagrams come out as a classify-ready batch: the reference continues with DecodeTCP / DecodeUDP /
 * the flow table on them (decode-ipv4.c:241-290), which ppe_classify / ppe_classify_flow of that batch reproduce
 * (their L2 / IPv4 checks pass by construction; the counters of that classify count the datagram once more).
 * The datagram's verdict applies to all of its fragments (the reference forwards or frees the chain with it).
 * Aging (Frag_defrag_timeout, decode-defrag.c:490-551, every second): ppe_defrag_age frees completed FCBs and those
 * idle for more than timeout_seconds (FRAG_MAX_TIMEOUT 20 s), dropping the fragments they still hold. */
enum ppe_defrag_status {
    PPE_DF_CACHED = 0,        /* held in its FCB's chain                                  STAT_FRAG_CACHE_OK   */
    PPE_DF_REASM = 1,         /* completed its datagram (dgram_of = its index)            STAT_FRAG_REASM_OK   */
    PPE_DF_SETUP_ERR = 2,     /* completed, but the reassembly buffer is too small: held  STAT_FRAG_SETUP_ERR  */
    PPE_DF_FCB_FULL = 3,      /* drop: fcb_max FCBs in use                                STAT_FRAG_FCB_FULL   */
    PPE_DF_HW2SW_ERR = 4,     /* drop: frame longer than frag_buf_bytes                   STAT_FRAG_HW2SW_ERR  */
    PPE_DF_DELETED = 5,       /* drop: its FCB already reassembled, awaiting aging (decode-defrag.c:422-427)    */
    PPE_DF_CACHE_FULL = 6,    /* drop: cache_max fragments already held                   STAT_FRAG_CACHE_FULL */
    PPE_DF_DEFRAG_ERR = 7,    /* drop: overlap / duplicate last fragment / short final    STAT_FRAG_DEFRAG_ERR */
    PPE_DF_NOT_FRAG = 8,      /* input is not an IPv4 fragment Defrag would see (caller error; untouched)      */
    PPE_DF__COUNT = 9
};
#define PPE_DF_TEARDROP 0x100u   /* | PPE_DF_DEFRAG_ERR: an overlap (DP_Teardrop_Attack_Monitor, decode-defrag.c:395-398) */

typedef struct {
    uint32_t fcb_max;          /* 0 → DEFRAG_FCB_MAX 1024 (decode-defrag.h:11)                                 */
    uint32_t cache_max;        /* 0 → defrag_cache_max 8 (decode-defrag.c:24); <= 16                           */
    uint32_t frag_buf_bytes;   /* 0 → 2024: the 2 KB small-buffer slice minus its 24-B control block
                                  (mem_pool.c:249, mem_pool.h:62); <= 4096                                     */
    uint32_t reasm_buf_bytes;  /* 0 → 8168: the 8 KB large-buffer slice minus its control block (mem_pool.c:269) */
    uint32_t max_batch;        /* fragments per ppe_defrag call; 0 → 65536                                      */
    uint32_t pad;
} ppe_defrag_cfg_t;

typedef struct {
    const uint8_t  *pkt;       /* whole frames, frame i at pkt + off[i] (device)                                 */
    const uint64_t *off;
    const uint32_t *len;       /* n × pkt_totallen                                                              */
    const uint64_t *id;        /* optional n × caller packet ids, echoed in dgram_frags (NULL → the batch index) */
    uint32_t        n;
    uint32_t        pad;
    uint64_t        now_seconds;   /* FCB_UPDATE_TIMESTAMP of every FCB the batch touches                       */
} ppe_frag_batch_t;

typedef struct {
    uint32_t *status;          /* n × (enum ppe_defrag_status | PPE_DF_TEARDROP)                                 */
    uint32_t *dgram_of;        /* optional n: datagram index of a PPE_DF_REASM fragment, else 0xffffffff        */
    uint8_t  *dgram_hdr;       /* n × hdr_stride: the first bytes of datagram j (a ppe_batch_t.hdr; zero-padded) */
    uint32_t *dgram_len;       /* n: its pkt_totallen (a ppe_batch_t.len); 0 for j >= the datagram count        */
    uint8_t  *dgram_pkt;       /* optional n × reasm_buf_bytes: the whole reassembled frames                    */
    uint64_t *dgram_frags;     /* optional n × cache_max: ids of datagram j's fragments in chain order, ~0 pad   */
                               /* (dgram_hdr / dgram_pkt / dgram_frags rows j >= the datagram count: not written) */
    uint32_t *n_dgram;         /* optional device word: datagrams written                                      */
    uint32_t  hdr_stride;      /* 64 or 128                                                                    */
    uint32_t  pad;
} ppe_defrag_out_t;

typedef struct {
    uint64_t running;          /* FCBs in use (fcb_running_num)                                                 */
    uint64_t new_fcb, del_fcb; /* decode-defrag.c:15-16                                                         */
    uint64_t st[PPE_DF__COUNT];/* fragments per enum ppe_defrag_status                                          */
    uint64_t teardrop;         /* overlaps among PPE_DF_DEFRAG_ERR                                              */
    uint64_t timeout_drop;     /* fragments dropped by ppe_defrag_age                                           */
    uint64_t datagrams;        /* reassembled datagrams emitted                                                 */
    uint32_t fcb_max, cache_max, frag_buf_bytes, reasm_buf_bytes, max_batch, slots;
} ppe_defrag_info_t;

typedef struct ppe_defrag_table ppe_defrag_t;
/* FragModule_init (decode-defrag.c:582-625): a device FCB table on ctx's device.  cfg may be NULL (defaults). */
int  ppe_defrag_create(ppe_ctx_t *ctx, const ppe_defrag_cfg_t *cfg, ppe_defrag_t **out);
int  ppe_defrag_destroy(ppe_defrag_t *d);                              /* FragModule_Release */
/* Defrag for a device-resident batch of fragments, stream-ordered on `stream` (batches in call order).
 * status, dgram_of and dgram_len are written for all n entries (dgram_len 0 past the datagram count: a runt frame
 * whose verdict does not depend on its window bytes), so a ppe_classify of {dgram_hdr, dgram_len, n, hdr_stride}
 * can follow on the same stream without a host sync. */
int  ppe_defrag(ppe_defrag_t *d, const ppe_frag_batch_t *in, const ppe_defrag_out_t *out, void *stream);
/* Frag_defrag_timeout: free FCBs that completed, or with now > last && now - last > timeout_seconds; the ids of
 * the fragments they still held go to dropped[0..max) (host; may be NULL), *n_dropped = their count, *n_freed =
 * FCBs freed (either may be NULL).  Synchronises. */
int  ppe_defrag_age(ppe_defrag_t *d, uint64_t now_seconds, uint64_t timeout_seconds, uint64_t *dropped,
                    uint32_t max, uint32_t *n_dropped, uint32_t *n_freed);
int  ppe_defrag_info(ppe_defrag_t *d, ppe_defrag_info_t *info);      /* synchronises */
/* How the last ppe_defrag batch of d ran, without synchronising: *kind 1 and *launches 1 for the one-launch kernel (a
 * batch of at most 4 fragments, the measured cutoff, runs its six phases in one workgroup; byte-identical outputs and
 * table state, and both shapes interleave freely on one table), *kind 0 and *launches 6 otherwise: a larger batch, a
 * table created with PPE_DEFRAG_SMALL=0 in the environment (the A/B switch), or the PPE_DF_LOOK_FAIL test hook armed.
 * (0, 0) before the first batch.  Diagnostic: PPE_DEFRAG_SMALL=N with N > 1 at ppe_defrag_create gives that table the
 * one launch up to min(N, 256) fragments, the kernel's workgroup, instead of the cutoff (for measuring and testing the
 * kernel past it: slower than six launches from 8 fragments on); unset or 1: the cutoff. */
int  ppe_defrag_launch_info(ppe_defrag_t *d, uint32_t *kind, uint32_t *launches);
/* ppe_defrag for a batch in host memory: every pointer of in and out is a host pointer (pageable or pinned), and
 * out->n_dgram is an optional host word.  The batch runs as consecutive ppe_defrag batches of `chunk` fragments
 * (0, or more than max_batch: max_batch) on one ordered stream of the table's own; datagram indices run on across
 * the chunks, and every output and ppe_defrag_info is the same whatever the chunk (ppe_defrag is one core's run in
 * index order and now_seconds is constant over the call).  Only status, dgram_of (n entries each) and the rows of the
 * datagrams that exist (dgram_len / dgram_hdr / dgram_pkt / dgram_frags rows below the count) are written.  in->id
 * NULL: the index in the whole batch.  Synchronises before it returns.  PPE_EINVAL for a missing required pointer or
 * a wrong hdr_stride, and PPE_EIO for a look-back error pending when the call begins: nothing is written on either.
 * A device error or a look-back error that a chunk of this call raises also returns PPE_EIO, with the outputs of the
 * chunks before it written. */
int  ppe_defrag_host(ppe_defrag_t *d, const ppe_frag_batch_t *in, const ppe_defrag_out_t *out, uint32_t chunk);

/* ---- Port-scan detector on the stateless classify path (dataplane/src/attack/dp_portscan.c) ----
 * The reference runs PortScan_Detect on every flow miss after syn_check and before the ACL (flow.c:215-230).  The
 * stateless path treats every packet as a miss, so with a table attached and able = 1, ppe_classify and
 * ppe_classify_batches run the detector for every packet that would reach the ACL (PPE_F_L4 set and not stopped by
 * syn_check), in batch index order, batches in call order (the batches of one ppe_classify_batches call count as
 * consecutive batches), with exactly the sequential semantics of one core:
 *   find the source's record by sip or create it (zeroed; a failed create, `capacity` records live, is NOMEM:
 *   the first capacity - live new sources by first appearance get records, every packet of the others is NOMEM);
 *   both set cycle = now_cycles (:109, :263); then PortScan_Detec_process (:139-210) verbatim: the hold test against
 *   mbuf->timestamp (batch.ts[i], or cfg->now_seconds without ts), last_dport == 0 as "first create", the three
 *   unsigned now - last_cycle branches (< rate; strictly between rate and 2 rate; everything else, which includes
 *   exactly rate, exactly 2 rate and a wrapped now < last_cycle), detection when last_exception >= exception_freq on
 *   a port change (hold = now_seconds + hold_seconds).
 * Any result but OK with action 0 makes the packet PPE_ST_PORTSCAN_DROP: FLOW_PROC_FAIL and OUT_DROP, no ACL counter,
 * no StreamTcp.  With action 1 the packet goes on to the ACL unchanged; detection and state still run.
 * The clock is the caller's: ppe_portscan_clock sets cvmx_get_cycle() and OCT_TIME_SECONDS_SINCE1970 for the batches
 * enqueued after it (by value, no synchronisation); rate (oct_cpu_rate) is cycles_per_second.
 * With a table attached and able = 1 every classify call of the context must go through one stream (or be ordered by
 * the caller), and ppe_classify_flow and ppe_classify_host return PPE_ENOTSUP before touching anything (the first:
 * the flow-table path calls the detector on flow misses only and has an attachment point of its own,
 * ppe_flow_portscan_attach below; the second: its chunks run on several streams; ppe_classify_host_ordered is the
 * host-buffer call that runs the detector).
 * The pre-pass of a batch of at most 2,048 packets is one kernel launch of one workgroup; a larger batch takes the
 * staged launches (ten, and more sort passes above 2,048 keys).  Both leave the same verdicts, counters and records.
 * PPE_PS_FUSED=0 in the environment at ppe_portscan_create gives a table that always takes the staged launches.
 * A new context has nothing attached: every output and counter is as without this interface. */
typedef struct {
    uint32_t able;               /* portscan_able (dp_portscan.c:10); 0/1                                         */
    uint32_t action;             /* portscan_action (:11): 0 drop, 1 forward                                       */
    uint32_t exception_freq;     /* portscan_exception_freq (:9)                                                   */
    uint32_t hold_seconds;       /* flood_hold_time (dp_attack.c:25)                                               */
    uint32_t capacity;           /* record pool; 0 = PORTSCAN_ITEM_NUM 100000 (dp_portscan.h:67)                    */
    uint32_t max_batch;          /* packets per batch; 0 = 1 << 20                                                 */
    uint64_t cycles_per_second;  /* oct_cpu_rate; 0 = 1000000000                                                   */
    uint64_t pad;
} ppe_portscan_cfg_t;

typedef struct {                 /* pcb_t (dp_portscan.h:25-35)                                                     */
    uint32_t sip;
    uint32_t last_dport;
    uint32_t exception, last_exception;
    uint64_t last_cycle, cycle, hold;
} ppe_portscan_entry_t;

typedef struct {
    uint64_t live;               /* records in use                                                                 */
    uint64_t new_pcb, del_pcb;   /* dp_portscan.c:12-13                                                            */
    uint64_t ok, nomem, detected, hold;   /* packets per PortScan_Detect result                                    */
    uint64_t drop;               /* attstat.portscan_drop (STAT_ATTACK_PORTSCAN_DROP, flow.c:226)                   */
    ppe_portscan_cfg_t cfg;      /* the configuration in force (defaults filled in)                                */
    uint32_t slots, rebuilds;    /* open-addressing slots; table rebuilds (aging, slot reclamation)                */
} ppe_portscan_info_t;

typedef struct ppe_portscan_table ppe_portscan_t;
/* PortScan_Module_init (dp_portscan.c:308-356).  cfg NULL = the reference defaults {1, 0, 50, 600, 0, 0, 0};
 * able / action above 1: PPE_EINVAL. */
int  ppe_portscan_create(ppe_ctx_t *ctx, const ppe_portscan_cfg_t *cfg, ppe_portscan_t **out);
int  ppe_portscan_destroy(ppe_portscan_t *ps);   /* detaches it from its context first */
int  ppe_portscan_attach(ppe_ctx_t *ctx, ppe_portscan_t *ps);   /* NULL detaches */
int  ppe_portscan_clock(ppe_portscan_t *ps, uint64_t now_cycles, uint64_t now_seconds);
/* able, action, exception_freq, hold_seconds live (dp_cmd.c:2133-2236); the other words are ignored */
int  ppe_portscan_set(ppe_portscan_t *ps, const ppe_portscan_cfg_t *cfg);
/* PortScan_timeout (:43-93): free every record with now > cycle && now - cycle > 20 * rate; *freed may be NULL.
 * Synchronises. */
int  ppe_portscan_age(ppe_portscan_t *ps, uint64_t now_cycles, uint64_t *freed);
int  ppe_portscan_info(ppe_portscan_t *ps, ppe_portscan_info_t *info);   /* synchronises */
/* Copy up to `max` records to host (table order); *n = records in use.  Synchronises. */
int  ppe_portscan_dump(ppe_portscan_t *ps, ppe_portscan_entry_t *entries, uint32_t max, uint32_t *n);
/* The pre-pass of the last batch enqueued with this table: *kind 1 the one-launch kernel, 0 the staged launches;
 * *launches the kernel launches it made (0 before the first batch).  Either pointer may be NULL.  No synchronisation. */
int  ppe_portscan_prepass_info(ppe_portscan_t *ps, uint32_t *kind, uint32_t *launches);
const char *ppe_portscan_last_error(ppe_portscan_t *ps);

/* ---- Port-scan detector on the flow-table path (flow.c:196-243) ----
 * The flow-table path's attachment point for the same table: with a table flow-attached and able = 1, ppe_classify_flow
 * and ppe_classify_flow_host run FlowGetFlowFromHash with PortScan_Detect inside, exactly as one core running the batch
 * in index order against both tables as the earlier packets left them:
 *   - a packet that finds its flow (in the table, or created by an earlier packet of the batch) is forwarded and
 *     accounted as without the detector and never reaches it: no record, no cycle stamp, no result count, even when
 *     its source is held;
 *   - a miss that fails syn_check is PPE_ST_FLOW_TCP_NO_SYN_FIRST, the detector is not called;
 *   - every other miss calls PortScan_Detect (the semantics above: its own sip and dport, batch.ts[i] or
 *     cfg->now_seconds, the table's clock; a record-less source gets a record at its first call while live < capacity,
 *     else that call and every later one of the source in the batch are NOMEM);
 *   - a result other than OK with action 0 is PPE_ST_PORTSCAN_DROP as the stateless path emits and counts it (acl_hit
 *     -1, PPE_F_ACL clear, flow hash and tuple kept; the RX_OK chain, FLOW_PROC_FAIL, OUT_DROP, the table's drop): no
 *     flow, no PPE_F_FLOW / NEWFLOW / TOCLIENT; with action 1 the state still runs and the packet goes on;
 *   - then the ACL's verdict: DROP is ACL_DROP with no flow, FW creates the flow (FlowAdd) or is PPE_ST_FLOW_NOMEM.
 * So a flow's creator is the lowest-index packet of its 5-tuple (either direction) that misses, passes syn_check, is
 * not dropped by the detector, is forwarded by the ACL and finds pool room.
 * One batch takes at most ppe_flow_portscan_max() packets (one launch of one workgroup, ppe_flow_launch_info kind 2);
 * a larger device batch returns PPE_ENOTSUP before anything is touched (ppe_classify_flow_host chunks host batches of
 * any size); n above the port-scan table's max_batch: PPE_EINVAL.  Also PPE_ENOTSUP before anything is touched: attack
 * monitors flow-attached at the same time unless ppe_flow_combine is on (below), and stream tracking.  With able = 0 or nothing flow-attached the flow path is
 * byte for byte what it is without this interface, at every size.  The stateless calls do not see a flow-attached table.
 * A table sits on at most one of the two attachment points: attaching one that the other point holds is PPE_EINVAL
 * (detach first), as is a table of another context; ppe_portscan_destroy detaches from whichever holds it. */
int  ppe_flow_portscan_attach(ppe_ctx_t *ctx, ppe_portscan_t *ps);   /* NULL detaches */
uint32_t ppe_flow_portscan_max(void);
/* Debug count (tools/ab_flow_portscan.py): the resolve rounds of the last batch that took the kernel with the detector
 * inside (0: none yet, or no packet of it was pending).  A plain flow batch (able 0, nothing flow-attached) does not
 * change it: check ppe_flow_launch_info for kind 2 first.  Synchronises. */
int  ppe_flow_portscan_rounds(ppe_ctx_t *ctx, uint32_t *rounds);
/* ---- The monitors and the detector together on the flow-table path: the reference's whole order, Decode -> DecodeIPV4 /
 * DecodeTCP (land, SYN-flood, SYN-count, UDP-flood monitors) -> FlowHandlePacket -> FlowFind | miss -> syn_check ->
 * PortScan_Detect -> DP_Acl_Lookup -> FlowAdd (syncount_accum) ----
 * 0 (a new context): ppe_classify_flow refuses a batch while a port-scan table with able 1 and attack monitors are both
 * flow-attached (PPE_ENOTSUP, as before).  1: such a batch runs the reference's whole path in one launch
 * (ppe_flow_launch_info kind 3), exactly as one core running the batch in index order, packet i seeing all three
 * states as packets 0..i-1 left them:
 *   - the monitors first, for every packet exactly as under ppe_flow_attack_attach alone: who reaches which monitor,
 *     statuses 25-28 and the row of a monitor drop, udp_accum / syn_accum, the hold arming, the port byte (entry 0 of
 *     ppe_attack_ports' table, none: port 0), the clock (ppe_attack_clock / _tick, not batch.ts).  A packet a monitor
 *     drops never reaches FlowHandlePacket: no lookup, no claim, no tombstone, no PortScan_Detect call, no record or
 *     cycle stamp for its source, and it is no candidate when the detector's records run out;
 *   - the survivors take the path of ppe_flow_portscan_attach unchanged (found / FLOW_TCP_NO_SYN_FIRST / PortScan_Detect
 *     / 24 / ACL_DROP / FlowAdd / FLOW_NOMEM, the detector's clock and batch.ts as there);
 *   - syncount_accum gets +1 on the packet's port only for a TCP SYN packet that ends with PPE_F_NEWFLOW: a SYN the
 *     detector drops counts in syn_accum (the monitor saw it) and not in syncount_accum; when a later SYN of its tuple
 *     creates the flow, the +1 goes to that later packet's port.
 * Refused before anything is touched, with the switch on, both attached and able 1: n > ppe_flow_portscan_max() and
 * stream tracking (PPE_ENOTSUP), n above the port-scan table's max_batch (PPE_EINVAL).  With the switch on and only one
 * of the two attached, or the table's able 0, nothing changes: the same kernels and ppe_flow_launch_info as without it.
 * The switch is the context's, like the attachments: ppe_flow_destroy leaves it.  Unchanged: ppe_classify_flow_host
 * refuses monitors flow-attached (ppe_classify_flow_host_ports takes them, and with the switch on the combination), the
 * steered multi-GPU path refuses either attachment.
 * on > 1: PPE_EINVAL.  No synchronisation: it applies to the ppe_classify_flow calls made after it. */
int  ppe_flow_combine(ppe_ctx_t *ctx, uint32_t on);


/* ---- Land, SYN-flood and UDP-flood monitors on the stateless classify path (dataplane/src/attack/dp_attack.c) ----
 * All state is per input port (attrule.*[input], attinfo.ai[input]; OCT_PHY_PORT_MAX = 4, oct-port.h:14).  Every
 * enable test of the reference is `== 1` (ATTACK_ENABLE), so a field holding 2 is off, and drop_pack == 1 means drop.
 * With an object attached, ppe_classify and ppe_classify_batches run, per packet:
 *   UDP (decode-ipv4.c:141-149, dp_attack.c:582-634), for every non-fragment protocol-17 packet that passed the IPv4
 *   checks, before DecodeUDP (a bad UDP header is counted and may be flood-dropped before its length is looked at):
 *     udp_accum++; flood_udp == 1 && drop_pack == 1 && (udp_flood_hold || udppps > udp_speed) → PPE_ST_ATTACK_UDPFLOOD
 *     (the speed branch sets udp_flood_hold = 1, udp_flood_hold_time = now_seconds + hold_seconds when not yet held);
 *   TCP SYN (decode-tcp.c:162-173), for a TCP packet that passed the three length checks with th_flags & 0x02 (a
 *   SYN|ACK counts): pd.land == 1 && sip == dip && pd.drop_pack == 1 → PPE_ST_ATTACK_LAND (not added to syn_accum);
 *     else syn_accum++; the hold / speed branches as for UDP with flood_syn, synpps, syn_speed →
 *     PPE_ST_ATTACK_SYNFLOOD; else syncount > syn_count && td.drop_pack == 1 → PPE_ST_ATTACK_SYNCOUNT (not gated by
 *     flood_syn).
 *   syncount_accum++ (FlowAdd, flow.c:151-154) for every TCP SYN packet whose status is PPE_ST_ACL_FW after the
 *   port-scan mask and before StreamTcp's verdict: on this path every packet that reaches FlowAdd is the first of its
 *   flow.  The decrements (stream-tcp.c:608,660, stream-tcp-session.c:70) belong to the session machine: on the
 *   flow-table path with ppe_flow_stream_monitors, not on this one.
 * Not judged and not counted: fragments, PPE_ST_WINDOW_PUNT, anything that fails before the IPv4 protocol dispatch,
 * a TCP packet that fails a length check or has no SYN.  A reassembled datagram classified afterwards counts once (the
 * reference adds one per fragment, dp_attack.c:586-601: a known difference).  ICMP never reaches its monitors in the
 * reference build, and the teardrop monitor is ppe_defrag's: their rule fields are stored and shown, not acted on.
 * A monitor drop counts in ppe_counters_t the RX_OK chain up to IPV4_RX_OK, OUT_DROP, PKTS and RX_BYTES; nothing of
 * UDP / TCP / ACL / FLOW.  A monitor-dropped packet never reaches the port-scan detector or StreamTcp.
 * Between two ticks everything a verdict reads is constant (the hold flags change only on a packet dropped either
 * way), so the verdicts equal one core's processing the packets in any order.
 * The clock (OCT_TIME_SECONDS_SINCE1970) is the caller's: ppe_attack_clock / ppe_attack_tick, not batch.ts.
 * ppe_attack_set, _tick and _clear_stat are tiny kernels enqueued on the stream of the context's latest classify call
 * (the legacy default stream before the first): ordered with the launches enqueued before and after, no
 * synchronisation.  The caller orders its classify calls (one stream), as with the port-scan table.
 * With an object attached ppe_classify_flow and ppe_classify_host return PPE_ENOTSUP before touching anything (the
 * flow-table path has an attachment point of its own, ppe_flow_attack_attach below).
 * A new context has nothing attached: every output and counter is as without this interface. */
#define PPE_ATTACK_PORTS 4
typedef struct {                 /* packet_detect (dp_attack.h:26-33) */
    uint32_t drop_pack, land, teardrop, pingdeath, pingdeath_value;
} ppe_attack_pd_t;
typedef struct {                 /* traffic_detect (dp_attack.h:35-48) */
    uint32_t drop_pack, flood_ping, ping_speed, last_ping_flood_time, flood_udp, udp_speed, last_udp_flood_time,
             flood_syn, syn_speed, last_syn_flood_time, syn_count;
} ppe_attack_td_t;
typedef struct {
    ppe_attack_pd_t pd[PPE_ATTACK_PORTS];
    ppe_attack_td_t td[PPE_ATTACK_PORTS];
    uint32_t hold_seconds;       /* flood_hold_time (dp_attack.c:25) */
    uint32_t pad;
} ppe_attack_cfg_t;
typedef struct {                 /* attack_info (dp_attack.h:73-89); the ping fields stay 0 */
    uint64_t pingpps, ping_accum, udppps, udp_accum, synpps, syn_accum, syncount, syncount_accum;
    uint64_t ping_flood_hold, ping_flood_hold_time, syn_flood_hold, syn_flood_hold_time, udp_flood_hold,
             udp_flood_hold_time;
} ppe_attack_port_t;
typedef struct {
    ppe_attack_cfg_t cfg;        /* the rules in force */
    ppe_attack_port_t ai[PPE_ATTACK_PORTS];
    uint64_t land_drop, udpflood_drop, synflood_drop, syncount_drop;   /* attstat.land / udpspeed / synspeed / syncount */
    uint64_t now_seconds;        /* the clock the next launch takes */
} ppe_attack_info_t;

typedef struct ppe_attack ppe_attack_t;
/* cfg NULL: all-zero rules and hold_seconds 600 (DP_Attack_Del_All, flood_hold_time) */
int  ppe_attack_create(ppe_ctx_t *ctx, const ppe_attack_cfg_t *cfg, ppe_attack_t **out);
/* detaches it from its context first.  Destroy the object before its context: it keeps a pointer to the context, and
 * ppe_ctx_destroy neither detaches nor destroys it (the same holds for ppe_portscan_destroy) */
int  ppe_attack_destroy(ppe_attack_t *atk);
int  ppe_attack_attach(ppe_ctx_t *ctx, ppe_attack_t *atk);        /* NULL detaches */
/* ---- The same monitors on the flow-table path (ppe_classify_flow), the reference's own order: Decode -> DecodeIPV4 /
 * DecodeTCP (monitors) -> FlowHandlePacket -> FlowFind | syn_check -> ACL -> FlowAdd ----
 * While an object is attached here, ppe_classify_flow runs the monitors above with two differences:
 *   - a packet a monitor drops never reaches FlowHandlePacket: no FlowFind, no slot claimed, no flow record, no
 *     FlowUpdate and no last-seen store (also for a packet of a live flow), no PPE_F_FLOW / TOCLIENT / NEWFLOW; it is
 *     not a miss.  Its outputs and counters are the stateless path's (status 25-28, drop, acl_hit -1, flow hash 0,
 *     PPE_F_L4 clear, PPE_F_TCP | PPE_F_SYN on 25-27, ports 0; the RX chain up to IPV4_RX_OK, then OUT_DROP).  The
 *     monitors see a packet whether or not its flow exists (a SYN of a live flow counts in syn_accum);
 *   - syncount_accum counts flow creations, as DP_Attack_SynCountMonitor in FlowAdd behind flow_item_alloc does
 *     (flow.c:120-158): +1 on the packet's port only for a TCP SYN packet that ends up with PPE_F_NEWFLOW.  Not a
 *     later SYN of the same 5-tuple in the batch, not a SYN of a live flow, not a creator refused with
 *     PPE_ST_FLOW_NOMEM, not an ACL drop or FLOW_TCP_NO_SYN_FIRST, not a UDP or non-SYN TCP packet that creates a flow.
 *     (The stateless path counts every forwarded SYN: there every packet is a flow miss.)
 * Everything else is as above: the tick, set, clock, info, clear_stat, the show texts, the hold arming.  syncount_accum's
 * decrements take the sessions as well (ppe_flow_stream_monitors).  Still not built: per-fragment counting, ICMP.
 * ppe_classify_flow is one batch per call: it reads entry 0 of ppe_attack_ports' table (NULL or none: port 0), at the
 * call, by value.  Calls go through one stream or are ordered by the caller; ppe_attack_set / _tick apply to the
 * launches enqueued after them, without a synchronise.
 * The context's stateless calls (ppe_classify, ppe_classify_batches, ppe_classify_host) do not see an object attached
 * here: they run the kernels without monitors.  An object is attached to at most one of the two points: attaching
 * one that the other point holds returns PPE_EINVAL ("detach first"), as does an object of another context.
 * ppe_attack_destroy detaches from whichever point holds the object; ppe_flow_destroy leaves the attachment (it is
 * the context's, like the table pointer).  ppe_classify_flow still returns PPE_ENOTSUP, before touching anything,
 * with stream tracking on, a port-scan table attached, or an object attached with ppe_attack_attach.  Also PPE_ENOTSUP:
 * a port-scan table flow-attached with able 1 at the same time, unless ppe_flow_combine is on. */
int  ppe_flow_attack_attach(ppe_ctx_t *ctx, ppe_attack_t *atk);   /* NULL detaches */
/* the rule file load / DP_Attack_Del_All / dp_attack_defend_time_set: the rules and hold_seconds (the state stays) */
int  ppe_attack_set(ppe_attack_t *atk, const ppe_attack_cfg_t *cfg);
int  ppe_attack_clock(ppe_attack_t *atk, uint64_t now_seconds);   /* by value with the launches enqueued afterwards */
/* DP_Attack_Info_Update (dp_attack.c:712-748; the reference runs it once a second, watchdog.c:117-122): per port
 * pps = accum, accum = 0; now >= hold_time clears both hold fields (also when nothing is held); sets the clock too */
int  ppe_attack_tick(ppe_attack_t *atk, uint64_t now_seconds);
/* Sticky: device array ports[k] holds one byte per packet, the input port of each packet of batch k of every later
 * classify call (ppe_classify: k = 0).  ports NULL, ports[k] NULL or k >= nbatch: port 0 for every packet.  The kernels
 * use port & 3, so nothing is indexed past four ports; values >= 4 are the caller's error.  nbatch <= 4096.
 * Not a hot-path call: it allocates a new device table and copies the pointers synchronously; the table it replaces
 * is freed once the launches enqueued before the call (on the classify stream) have completed. */
int  ppe_attack_ports(ppe_attack_t *atk, const uint8_t *const *ports, uint32_t nbatch);
int  ppe_attack_info(ppe_attack_t *atk, ppe_attack_info_t *info);   /* synchronises */
int  ppe_attack_clear_stat(ppe_attack_t *atk);                      /* the four drop totals only */
const char *ppe_attack_last_error(ppe_attack_t *atk);
/* `show attack stat` text (dp_show_attack_stat, dp_cmd.c:2394-2529) byte for byte; snprintf semantics */
int  ppe_format_attack_stat(const ppe_attack_info_t *info, char *buf, size_t cap);
/* The Decode shim's rule-file load (ppe_decode.h, flow_attack_able; declared here because it takes the rule type): the
 * rules of the shim's monitor object become *cfg, except hold_seconds, which is the global flood_hold_time; the object
 * is created if need be.  The counts, holds and drop totals stay.  Takes the shim's lock.  PPE_ENODEV without a
 * context (DP_Acl_Rule_Init), PPE_EINVAL for NULL.  The /data/protection.rul parser is the caller's. */
int DP_Attack_Rule_Set(const ppe_attack_cfg_t *cfg);

/* `show packet statistic` / `show flow statistic` text (dp_show_pkt_stat / dp_show_flow_stat,
 * dataplane/src/common/dp_cmd.c:844-1818, 2346-2392) into buf (NUL-terminated, truncated to cap); returns the full
 * length.  The _ex forms take the IPv4 reassembly table's counters (NULL: those lines print 0, as the plain forms
 * do): the ip_frag_stat section, the new / del fcb lines and, while the teardrop monitor is enabled
 * (teardrop_monitor != 0; off in the reference's default configuration), the attack section's teardrop line. */
int  ppe_format_pkt_stat(const ppe_counters_t *c, char *buf, size_t cap);
int  ppe_format_flow_stat(const ppe_flow_info_t *f, char *buf, size_t cap);
int  ppe_format_pkt_stat_ex(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor, char *buf,
                            size_t cap);
int  ppe_format_flow_stat_ex(const ppe_flow_info_t *f, const ppe_defrag_info_t *df, char *buf, size_t cap);
/* ppe_format_pkt_stat_ex with the attack section's portscan_drop line from ps_info->drop (NULL: 0, as _ex prints) */
int  ppe_format_pkt_stat_ps(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor,
                            const ppe_portscan_info_t *ps_info, char *buf, size_t cap);
/* the four port-scan lines of `show fw config` (dp_cmd.c:2578-2590): detect stat, detect action, flood hold time,
 * portscan_exception_freq.  cfg NULL = the reference defaults. */
int  ppe_format_fw_config(const ppe_portscan_cfg_t *cfg, char *buf, size_t cap);
/* ppe_format_pkt_stat_ps with the attack section's land_drop / udp flood drop / syn flood drop / syncount lines from
 * atk_info's drop totals (NULL: 0, as the older forms print) */
int  ppe_format_pkt_stat_atk(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor,
                             const ppe_portscan_info_t *ps_info, const ppe_attack_info_t *atk_info, char *buf,
                             size_t cap);
const char *ppe_defrag_last_error(ppe_defrag_t *d);

/* Human-readable last error of this context (static storage of the ctx). */
const char *ppe_last_error(ppe_ctx_t *ctx);

/* Host-side classifier compiler (no device needed): rule list → image words (ppe_image.h layout, malloc'd;
 * free with ppe_acl_free_image).  binth = max rules in a leaf list before splitting (0 → default 1). */
int  ppe_acl_build_image(const RCP_BLOCK_ACL_RULE_TUPLE *rules, const uint8_t *used, uint32_t n,
                         uint32_t default_action, uint32_t binth, uint32_t **words, uint32_t *n_words,
                         ppe_acl_stats_t *stats);
void ppe_acl_free_image(uint32_t *words);

#ifdef __cplusplus
}
#endif
#endif /* PPE_HIP_H */
