/*
 * ppe_stat.c — the text of the reference's `show packet statistic` and `show flow statistic` commands
 * (dp_show_pkt_stat, dataplane/src/common/dp_cmd.c:844-1818; dp_show_flow_stat, :2346-2392), produced from this
 * engine's per-reason counters (ppe_counters_read) and flow-table totals (ppe_flow_info).
 *
 * Sections, line names and order follow the reference.  The ip_frag_stat lines, the attack section's teardrop line and
 * the flow text's fcb lines come from the IPv4 reassembly table (ppe_defrag_info) when one is given to the _ex forms:
 * fragments per Defrag outcome are exactly the STAT_FRAG_* increments of decode-defrag.c (cache_ok :391, reasm_ok
 * :279, setup_err :282, fcb_full :80, hw2sw_err :418, cache_full :437, defrag_err :401; fcb_no :87 is a memory-pool
 * failure the device table cannot have, out_oversize is commented out at :285), new / del fcb are :481 / :526, and
 * teardrop is counted only while the teardrop monitor is enabled (DP_Teardrop_Attack_Monitor, dataplane/src/attack/
 * dp_attack.c:487-498; disabled in the default configuration).  Lines whose counter has no source on the GPU path
 * print 0: the receive-error / from-linux / address counters of the Octeon I/O layer, ARP / ICMP / OSPF hand-offs to
 * Linux, TX, the other attack monitors (pass-through at default configuration), and output_* (the reference's
 * SELF_TEST build forwards without STAT_OUTPUT_*, flow.c:21,376-377).
 */
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ppe_hip.h"

#define NONE (-1)
/* reassembly-table sources (ppe_defrag_info_t), printed 0 without one */
#define DF(st) (1000 + (st))   /* fragments with Defrag outcome st */
#define DF_TEARDROP 2000       /* overlaps, while the teardrop monitor is enabled */
#define ATK(i) (4000 + (i))     /* drop total i of the attack monitors (ppe_attack_info_t: land, udp, syn, syncount), 0 without */
#define PS_DROP 3000           /* attstat.portscan_drop of a port-scan table (ppe_portscan_info_t), printed 0 without one */

typedef struct {
    const char *name;  /* printed as "<name>: %ld" */
    int counter;       /* enum ppe_counter, or NONE */
} stat_line_t;

typedef struct {
    const char *title;
    const stat_line_t *lines;
    int n;
    int blank_after;   /* the reference prints an empty line after most sections */
} stat_section_t;

/* dp_cmd.c:866-917 */
static const stat_line_t k_recv[] = {{"recv_packet_count", PPE_C_PKTS}, {"recv_packet_bytes", PPE_C_RX_BYTES},
                                     {"recv_packet_count_sum", PPE_C_PKTS}, {"recv_packet_bytes_sum", PPE_C_RX_BYTES}};
/* :923-992 (oct-rxtx.c:160-222: every packet here arrived through a hardware port) */
static const stat_line_t k_rx[] = {{"grp_err", NONE},          {"rx_fromhwport_err", NONE}, {"rx_fromlinux_err", NONE},
                                   {"rx_fromhwport_ok", PPE_C_PKTS}, {"rx_fromlinux_ok", NONE}, {"addr_err", NONE}};
static const stat_line_t k_ether[] = {{"headerlen_err", PPE_C_L2_HEADERLEN_ERR}, {"unsupport", PPE_C_L2_UNSUPPORT},
                                      {"rx_ok", PPE_C_L2_RX_OK}, {"arp_se2linux_ok", NONE},
                                      {"arp_se2linux_fail", NONE}};
static const stat_line_t k_vlan[] = {{"headerlen_err", PPE_C_VLAN_HEADERLEN_ERR},
                                     {"vlanlayer_exceed", PPE_C_VLAN_LAYER_EXCEED},
                                     {"unsupport", PPE_C_VLAN_UNSUPPORT}, {"rx_ok", PPE_C_VLAN_RX_OK},
                                     {"arp_se2linux_fail", NONE}, {"arp_se2linux_ok", NONE}};
static const stat_line_t k_ipv4[] = {{"headerlen_err", PPE_C_IPV4_HEADERLEN_ERR}, {"version_err", PPE_C_IPV4_VERSION_ERR},
                                     {"pktlen_err", PPE_C_IPV4_PKTLEN_ERR},     {"unsupport", PPE_C_IPV4_UNSUPPORT},
                                     {"rx_ok", PPE_C_IPV4_RX_OK},               {"icmp_se2linux_ok", NONE},
                                     {"icmp_se2linux_fail", NONE},              {"ospf_se2linux_ok", NONE},
                                     {"ospf_se2linux_fail", NONE}};
static const stat_line_t k_frag[] = {{"fraglen_err", PPE_C_FRAG_FRAGLEN_ERR}, {"fcb_no", NONE},
                                     {"hw2sw_err", DF(PPE_DF_HW2SW_ERR)}, {"fcb_full", DF(PPE_DF_FCB_FULL)},
                                     {"cache_full", DF(PPE_DF_CACHE_FULL)}, {"defrag_err", DF(PPE_DF_DEFRAG_ERR)},
                                     {"setup_err", DF(PPE_DF_SETUP_ERR)}, {"out_oversize", NONE},
                                     {"cache_ok", DF(PPE_DF_CACHED)}, {"reasm_ok", DF(PPE_DF_REASM)}};
static const stat_line_t k_icmp[] = {{"rx_ok", NONE}, {"drop", NONE}};
static const stat_line_t k_tcp[] = {{"headerlen_err", PPE_C_TCP_HEADERLEN_ERR}, {"pktlen_err", PPE_C_TCP_PKTLEN_ERR},
                                    {"rx_ok", PPE_C_TCP_RX_OK}};
static const stat_line_t k_udp[] = {{"headerlen_err", PPE_C_UDP_HEADERLEN_ERR}, {"pktlen_err", PPE_C_UDP_PKTLEN_ERR},
                                    {"rx_ok", PPE_C_UDP_RX_OK}};
static const stat_line_t k_acl[] = {{"drop", PPE_C_ACL_DROP}, {"fw", PPE_C_ACL_FW}};
static const stat_line_t k_flow[] = {{"node_nomem", PPE_C_FLOW_NODE_NOMEM}, {"proc_ok", PPE_C_FLOW_PROC_OK},
                                     {"proc_fail", PPE_C_FLOW_PROC_FAIL}, {"proc_drop", NONE},
                                     {"tcp_no_syn_first", PPE_C_FLOW_TCP_NO_SYN_FIRST}};
static const stat_line_t k_out[] = {{"output_fw", NONE}, {"output_drop", NONE}, {"output_cache", NONE},
                                    {"output_unsupport", NONE}};
static const stat_line_t k_tx[] = {{"port_err", NONE}, {"hw_send_err", NONE}, {"sw_desc_err", NONE},
                                   {"sw_send_err", NONE}, {"send_over", NONE}};
static const stat_line_t k_att[] = {{"land_drop", ATK(0)}, {"teardrop", DF_TEARDROP}, {"pingdeath", NONE},
                                    {"ping flood drop", NONE}, {"udp flood drop", ATK(1)}, {"syn flood drop", ATK(2)},
                                    {"syncount", ATK(3)}, {"portscan_drop", PS_DROP}};

#define SEC(t, a, b) {t, a, (int)(sizeof a / sizeof a[0]), b}
static const stat_section_t k_sections[] = {
    SEC("recv_count", k_recv, 1), SEC("rx_stat", k_rx, 1),     SEC("ether_stat", k_ether, 1),
    SEC("vlan_stat", k_vlan, 1),  SEC("ipv4_stat", k_ipv4, 1), SEC("ip_frag_stat", k_frag, 1),
    SEC("icmp_stat", k_icmp, 1),  SEC("tcp_stat", k_tcp, 1),   SEC("udp_stat", k_udp, 1),
    SEC("acl_stat", k_acl, 1),    SEC("flow_stat", k_flow, 1), SEC("output", k_out, 0),
    SEC("tx_stat", k_tx, 0),      SEC("attack stat", k_att, 1),
};

typedef struct {
    char *buf;
    size_t cap, len;
} out_t;

static void put(out_t *o, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const size_t room = o->len < o->cap ? o->cap - o->len : 0;
    const int k = vsnprintf(o->buf ? o->buf + o->len : NULL, o->buf ? room : 0, fmt, ap);
    va_end(ap);
    if (k > 0) o->len += (size_t)k;
}

static long line_value(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor,
                       const ppe_portscan_info_t *ps, const ppe_attack_info_t *atk, int ci) {
    if (ci == NONE) return 0L;
    if (ci >= 4000) {
        if (!atk) return 0L;
        const uint64_t v[4] = {atk->land_drop, atk->udpflood_drop, atk->synflood_drop, atk->syncount_drop};
        return (long)v[ci - 4000];
    }
    if (ci == PS_DROP) return ps ? (long)ps->drop : 0L;
    if (ci == DF_TEARDROP) return df && teardrop_monitor ? (long)df->teardrop : 0L;
    if (ci >= 1000) return df ? (long)df->st[ci - 1000] : 0L;
    return (long)c->c[ci];
}

int ppe_format_pkt_stat(const ppe_counters_t *c, char *buf, size_t cap) {
    return ppe_format_pkt_stat_ex(c, NULL, 0, buf, cap);
}

int ppe_format_pkt_stat_ex(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor, char *buf,
                           size_t cap) {
    return ppe_format_pkt_stat_ps(c, df, teardrop_monitor, NULL, buf, cap);
}

int ppe_format_pkt_stat_ps(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor,
                           const ppe_portscan_info_t *ps_info, char *buf, size_t cap) {
    return ppe_format_pkt_stat_atk(c, df, teardrop_monitor, ps_info, NULL, buf, cap);
}

int ppe_format_pkt_stat_atk(const ppe_counters_t *c, const ppe_defrag_info_t *df, int teardrop_monitor,
                            const ppe_portscan_info_t *ps_info, const ppe_attack_info_t *atk_info, char *buf,
                            size_t cap) {
    if (!c) return PPE_EINVAL;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "packet statistic:\n");
    put(&o, "----------------------------------\n");
    put(&o, "\n");
    for (size_t s = 0; s < sizeof k_sections / sizeof k_sections[0]; s++) {
        const stat_section_t *sec = &k_sections[s];
        put(&o, "%s:\n", sec->title);
        put(&o, "----------------\n");
        for (int i = 0; i < sec->n; i++) {
            const int ci = sec->lines[i].counter;
            put(&o, "%s: %ld\n", sec->lines[i].name, line_value(c, df, teardrop_monitor, ps_info, atk_info, ci));
        }
        put(&o, "----------------\n");
        if (sec->blank_after) put(&o, "\n");
    }
    return (int)o.len;
}

/* `show attack stat` (dp_show_attack_stat, dp_cmd.c:2394-2529): the rules and the monitor state of the four
 * interfaces, same format strings (%d for the rule words, %ld for the state) */
int ppe_format_attack_stat(const ppe_attack_info_t *info, char *buf, size_t cap) {
    if (!info) return PPE_EINVAL;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "attack rule:\n");
    for (int i = 0; i < PPE_ATTACK_PORTS; i++) {
        const ppe_attack_pd_t *pd = &info->cfg.pd[i];
        const ppe_attack_td_t *td = &info->cfg.td[i];
        const ppe_attack_port_t *ai = &info->ai[i];
        put(&o, "----------------\n");
        put(&o, "interface %d:\n", i);
        put(&o, "packet detect:\n");
        put(&o, "drop_pack: %d\n", (int)pd->drop_pack);
        put(&o, "land: %d\n", (int)pd->land);
        put(&o, "teardrop: %d\n", (int)pd->teardrop);
        put(&o, "pingdeath: %d\n", (int)pd->pingdeath);
        put(&o, "pingdeath_value: %d\n", (int)pd->pingdeath_value);
        put(&o, "\n");
        put(&o, "traffic detect:\n");
        put(&o, "drop_pack: %d\n", (int)td->drop_pack);
        put(&o, "flood_ping: %d\n", (int)td->flood_ping);
        put(&o, "ping_speed: %d\n", (int)td->ping_speed);
        put(&o, "flood_udp: %d\n", (int)td->flood_udp);
        put(&o, "udp_speed: %d\n", (int)td->udp_speed);
        put(&o, "flood_syn: %d\n", (int)td->flood_syn);
        put(&o, "syn_speed: %d\n", (int)td->syn_speed);
        put(&o, "syn_count: %d\n", (int)td->syn_count);
        put(&o, "\n");
        put(&o, "attack monitor info:\n");
        put(&o, "pingpps: %ld\n", (long)ai->pingpps);
        put(&o, "ping_accum: %ld\n", (long)ai->ping_accum);
        put(&o, "udppps: %ld\n", (long)ai->udppps);
        put(&o, "udp_accum: %ld\n", (long)ai->udp_accum);
        put(&o, "synpps: %ld\n", (long)ai->synpps);
        put(&o, "syn_accum: %ld\n", (long)ai->syn_accum);
        put(&o, "syncount: %ld\n", (long)ai->syncount);
        put(&o, "syncount_accum: %ld\n", (long)ai->syncount_accum);
    }
    put(&o, "----------------------------\n");
    return (int)o.len;
}

/* the port-scan lines of `show fw config` (dp_cmd.c:2578-2590), same format strings */
int ppe_format_fw_config(const ppe_portscan_cfg_t *cfg, char *buf, size_t cap) {
    const ppe_portscan_cfg_t ref = {1u, 0u, 50u, 600u, 0u, 0u, 0u, 0u}; /* dp_portscan.c:9-11, dp_attack.c:25 */
    const ppe_portscan_cfg_t *v = cfg ? cfg : &ref;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "portscan attack detect stat: %s\n", v->able ? "enable" : "disable");
    put(&o, "portscan attack detect action: %s\n", v->action ? "fw" : "drop");
    put(&o, "flood hold time: %d\n", (int)v->hold_seconds);
    put(&o, "portscan_exception_freq: %d\n", (int)v->exception_freq);
    return (int)o.len;
}

/* `show tcpstream statistic` (dp_show_tcpstream_stat, dp_cmd.c:174-842): the tcpstreamtrackstat lines, then the
 * tcpstreamreasmstat lines, in the reference's order.  The stateless path produces the six counters with a source
 * below (the two *_DISABLE drop reasons are counted, ppe_stream_counters_t, but the reference prints no line for
 * them); the session state machine's and the reassembly's lines print 0. */
static const stat_line_t k_tcpstream[] = {
    {"SYN_ACK_COUNT", PPE_SC_SYN_ACK_COUNT}, {"SYN_COUNT", PPE_SC_SYN_COUNT}, {"RST_COUNT", PPE_SC_RST_COUNT},
    {"RST_BUT_NO_SESSION", PPE_SC_RST_BUT_NO_SESSION}, {"FIN_BUT_NO_SESSION", PPE_SC_FIN_BUT_NO_SESSION},
    {"SESSION_NO_MEM", NONE}, {"FIN_INVALID_ACK", NONE}, {"FIN_OUT_OF_WINDOW", NONE}, {"SESSION_PARAM_ERR", NONE},
    {"WHS3_SYNACK_TOSERVER_SYN_RECV", NONE}, {"WHS3_SYNACK_SEQ_MISMATCH", NONE},
    {"WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK", NONE}, {"WHS3_SYN_TOCLIENT_ON_SYN_RECV", NONE},
    {"WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV", NONE}, {"WHS3_SYNACK_IN_WRONG_DIRECTION", NONE},
    {"WHS3_ACK_IN_WRONG_DIR", NONE}, {"WHS3_RIGHT_SEQ_WRONG_ACK_EVASION", NONE}, {"WHS3_WRONG_SEQ_WRONG_ACK", NONE},
    {"WHS3_ASYNC_WRONG_SEQ", NONE}, {"WHS3_SYNACK_WITH_WRONG_ACK", NONE}, {"WHS4_WRONG_SEQ", NONE},
    {"WHS4_INVALID_ACK", NONE}, {"WHS4_SYNACK_WITH_WRONG_ACK", NONE}, {"WHS4_SYNACK_WITH_WRONG_SYN", NONE},
    {"EST_INVALID_ACK", NONE}, {"EST_PKT_BEFORE_LAST_ACK", NONE}, {"EST_PACKET_OUT_OF_WINDOW", NONE},
    {"EST_SYNACK_RESEND", NONE}, {"EST_SYNACK_TOSERVER", NONE}, {"EST_SYNACK_RESEND_WITH_DIFFERENT_ACK", NONE},
    {"EST_SYNACK_RESEND_WITH_DIFF_SEQ", NONE}, {"EST_SYN_TOCLIENT", NONE}, {"EST_SYN_RESEND_DIFF_SEQ", NONE},
    {"EST_SYN_RESEND", NONE}, {"PKT_RETRANSMISSION", NONE}, {"FIN2_FIN_WRONG_SEQ", NONE}, {"FIN2_INVALID_ACK", NONE},
    {"FIN2_ACK_WRONG_SEQ", NONE}, {"FIN1_FIN_WRONG_SEQ", NONE}, {"FIN1_INVALID_ACK", NONE},
    {"FIN1_ACK_WRONG_SEQ", NONE}, {"SHUTDOWN_SYN_RESEND", NONE}, {"CLOSEWAIT_FIN_OUT_OF_WINDOW", NONE},
    {"CLOSING_ACK_WRONG_SEQ", NONE}, {"CLOSEWAIT_INVALID_ACK", NONE}, {"CLOSING_INVALID_ACK", NONE},
    {"CLOSEWAIT_PKT_BEFORE_LAST_ACK", NONE}, {"CLOSEWAIT_ACK_OUT_OF_WINDOW", NONE}, {"LASTACK_ACK_WRONG_SEQ", NONE},
    {"LASTACK_INVALID_ACK", NONE}, {"TIMEWAIT_ACK_WRONG_SEQ", NONE}, {"TIMEWAIT_INVALID_ACK", NONE},
    {"PKT_INVALID_ACK", NONE}, {"PKT_BAD_WINDOW_UPDATE", NONE}, {"PKT_BROKEN_ACK", PPE_SC_PKT_BROKEN_ACK},
    {"REASM_BEFORE_RA_BASE", NONE}, {"REASM_SEG_NO_MEM", NONE}, {"REASM_HW2SW_ERR", NONE}, {"REASM_CACHE", NONE},
    {"REASM_NO_NEED_REASM", NONE}, {"REASM_SETUP_FAIL", NONE}, {"REASM_OK", NONE}, {"REASM_OVERLAP", NONE}};

int ppe_format_tcpstream_stat(const ppe_stream_counters_t *c, const ppe_stream_tcp_cfg_t *cfg, char *buf, size_t cap) {
    if (!c) return PPE_EINVAL;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "tcpstream statistic:\n");
    put(&o, "tcpstream track: %s\n", cfg && cfg->track ? "enable" : "disable");
    put(&o, "tcpstream reasm: %s\n", cfg && cfg->reasm ? "enable" : "disable");
    put(&o, "----------------------------------\n");
    for (size_t i = 0; i < sizeof k_tcpstream / sizeof k_tcpstream[0]; i++) {
        const int ci = k_tcpstream[i].counter;
        put(&o, "%s: %ld\n", k_tcpstream[i].name, ci == NONE ? 0L : (long)c->c[ci]);
    }
    put(&o, "----------------\n");
    put(&o, "\n");
    return (int)o.len;
}

/* the same text from the session path's block (ppe_stream_track_counters_t: all 58 fields of tcpstream_track_stat in
 * the struct's order): every track line from the field of its own name, the reassembly lines 0 */
static const char *const k_stc_names[PPE_STC__COUNT] = {
    "SYN_ACK_COUNT", "SYN_COUNT", "RST_COUNT", "RST_BUT_NO_SESSION", "FIN_BUT_NO_SESSION",
    "MIDSTREAM_OR_ONESIDE_DISABLE", "MIDSTREAM_DISABLE", "ONESIDE_DISABLE", "SESSION_NO_MEM", "FIN_INVALID_ACK",
    "FIN_OUT_OF_WINDOW", "SESSION_PARAM_ERR", "WHS3_SYNACK_TOSERVER_SYN_RECV", "WHS3_SYNACK_SEQ_MISMATCH",
    "WHS3_SYNACK_RESEND_WITH_DIFFERENT_ACK", "WHS3_SYN_TOCLIENT_ON_SYN_RECV", "WHS3_SYN_RESEND_DIFF_SEQ_ON_SYN_RECV",
    "WHS3_SYNACK_IN_WRONG_DIRECTION", "WHS3_ACK_IN_WRONG_DIR", "WHS3_RIGHT_SEQ_WRONG_ACK_EVASION",
    "WHS3_WRONG_SEQ_WRONG_ACK", "WHS3_ASYNC_WRONG_SEQ", "WHS3_SYNACK_WITH_WRONG_ACK", "WHS4_WRONG_SEQ",
    "WHS4_INVALID_ACK", "WHS4_SYNACK_WITH_WRONG_ACK", "WHS4_SYNACK_WITH_WRONG_SYN", "EST_INVALID_ACK",
    "EST_PKT_BEFORE_LAST_ACK", "EST_PACKET_OUT_OF_WINDOW", "EST_SYNACK_RESEND", "EST_SYNACK_TOSERVER",
    "EST_SYNACK_RESEND_WITH_DIFFERENT_ACK", "EST_SYNACK_RESEND_WITH_DIFF_SEQ", "EST_SYN_TOCLIENT",
    "EST_SYN_RESEND_DIFF_SEQ", "EST_SYN_RESEND", "PKT_RETRANSMISSION", "FIN2_FIN_WRONG_SEQ", "FIN2_INVALID_ACK",
    "FIN2_ACK_WRONG_SEQ", "FIN1_FIN_WRONG_SEQ", "FIN1_INVALID_ACK", "FIN1_ACK_WRONG_SEQ", "SHUTDOWN_SYN_RESEND",
    "CLOSEWAIT_FIN_OUT_OF_WINDOW", "CLOSING_ACK_WRONG_SEQ", "CLOSEWAIT_INVALID_ACK", "CLOSING_INVALID_ACK",
    "CLOSEWAIT_PKT_BEFORE_LAST_ACK", "CLOSEWAIT_ACK_OUT_OF_WINDOW", "LASTACK_ACK_WRONG_SEQ", "LASTACK_INVALID_ACK",
    "TIMEWAIT_ACK_WRONG_SEQ", "TIMEWAIT_INVALID_ACK", "PKT_INVALID_ACK", "PKT_BAD_WINDOW_UPDATE", "PKT_BROKEN_ACK"};

int ppe_format_tcpstream_stat_ex(const ppe_stream_track_counters_t *c, const ppe_stream_tcp_cfg_t *cfg, char *buf,
                                 size_t cap) {
    if (!c) return PPE_EINVAL;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "tcpstream statistic:\n");
    put(&o, "tcpstream track: %s\n", cfg && cfg->track ? "enable" : "disable");
    put(&o, "tcpstream reasm: %s\n", cfg && cfg->reasm ? "enable" : "disable");
    put(&o, "----------------------------------\n");
    for (size_t i = 0; i < sizeof k_tcpstream / sizeof k_tcpstream[0]; i++) {
        long v = 0;
        for (int k = 0; k < PPE_STC__COUNT; k++)
            if (strcmp(k_tcpstream[i].name, k_stc_names[k]) == 0) v = (long)c->c[k];
        put(&o, "%s: %ld\n", k_tcpstream[i].name, v);
    }
    put(&o, "----------------\n");
    put(&o, "\n");
    return (int)o.len;
}

int ppe_format_flow_stat(const ppe_flow_info_t *f, char *buf, size_t cap) {
    return ppe_format_flow_stat_ex(f, NULL, buf, cap);
}

int ppe_format_flow_stat_ex(const ppe_flow_info_t *f, const ppe_defrag_info_t *df, char *buf, size_t cap) {
    if (!f) return PPE_EINVAL;
    out_t o = {buf, buf ? cap : 0, 0};
    if (buf && cap) buf[0] = 0;
    put(&o, "new flow is: %ld\ndel flow is: %ld\n", (long)f->new_flow, (long)f->del_flow);
    /* FCBs created / freed by the reassembly table (new_fcb / del_fcb, decode-defrag.c:15-16,481,526) */
    put(&o, "new fcb is: %ld\ndel fcb is: %ld\n", df ? (long)df->new_fcb : 0L, df ? (long)df->del_fcb : 0L);
    put(&o, "new pcb is: %ld\ndel pcb is: %ld\n", 0L, 0L);
    return (int)o.len;
}
