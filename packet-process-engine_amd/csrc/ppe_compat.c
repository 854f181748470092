/*
 * ppe_compat.c — the reference's decoder / ACL / plugin / log entry points as thin shims over the GPU engine.
 *
 *   DP_Acl_Rule_Init        main.c:177
 *   DP_Acl_Load_Rule        dataplane/src/common/dp_cmd.c:2019 (builds the back classifier; published when
 *                           g_acltree_running names its unit_tree_t, set_running_acltree, dp_cmd.c:1980-1985)
 *   DP_Acl_Rule_Clean       dataplane/src/common/dp_cmd.c:2030
 *   DP_Acl_Rule_Release     dataplane/src/platform/oct-init.c:755
 *   DP_Acl_Rule_Commit      the dp_acl_rule_commit protocol, dataplane/src/common/dp_cmd.c:1987-2053
 *   DP_Acl_Lookup           dataplane/src/flow/flow.c:232
 *   Decode                  dataplane/src/decode/decode.c:19-28 (synchronous by default, burst-queued on request;
 *                           see ppe_decode.h)
 *   reg_fw_alert/DP_Log_Func dataplane/src/common/dp_log.c:12-31
 *   plugin_modules          dataplane/src/plugin/plugin-mod/plugin.c:8
 * Every packet decision is made by the HIP kernels; nothing here inspects packet bytes to classify them.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "ppe_decode.h"
#include "ppe_hip.h"

uint32_t dp_acl_action_default = ACL_RULE_ACTION_DROP;
int gWstDepth = 0, gAvgDepth = 0, gChildCount = 0, gNumTreeNode = 0, gNumLeafNode = 0;
uint32_t unsupport_proto_action = 0; /* dataplane/src/common/dp_cmd.c:37 */
uint32_t syn_check = 1;              /* dataplane/src/flow/flow.c:26 */
/* StreamTcp's settings (dataplane/src/plugin/stream-tcp/stream-tcp.c:16,20-21), read per classify call.  The reference
 * starts with tracking on; this library starts with it OFF, so that a dataplane linked against it keeps the verdicts
 * it had: set stream_tcp_track_enable = 1 for the reference's default behaviour. */
uint32_t stream_tcp_track_enable = 0;
uint32_t stream_tcp_midstream = 0;
uint32_t stream_tcp_async_oneside = 0;
/* The port-scan detector's settings (dataplane/src/attack/dp_portscan.c:9-11, dp_attack.c:25), read per classify call.
 * The reference starts with portscan_able = 1; this library starts with it OFF, like StreamTcp above: set
 * portscan_able = 1 for the reference's default behaviour. */
uint32_t portscan_able = 0;
uint32_t portscan_action = 0;
uint32_t portscan_exception_freq = 50;
uint32_t flood_hold_time = 600;
/* The flow table behind Decode (FlowHandlePacket, flow.c:181-310), read per classify call.  The reference has no such
 * switch (every packet goes through its table); this library starts with it OFF, like the two above: set
 * flow_able = 1 for the reference's behaviour.  flow_item_num: the pool (MEM_POOL_FLOW_NODE_NUM, mem_pool.h:72), read
 * when the table is created. */
uint32_t flow_able = 0;
/* PortScan_Detect on the flow table's misses (flow.c:215-230): off until set, with flow_able == 1 only (ppe_decode.h) */
uint32_t flow_portscan_able = 0;
/* The land / SYN-flood / SYN-count / UDP-flood monitors ahead of the flow table (decode-ipv4.c:141-149,
 * decode-tcp.c:162-173, flow.c:151-154): off until set, with flow_able == 1 only (ppe_decode.h) */
uint32_t flow_attack_able = 0;
uint32_t flow_item_num = 100000;
/* Defrag behind Decode (decode-ipv4.c:102-125, decode-defrag.c:449-487), read per flush.  The reference has no such
 * switch (DecodeIPV4 always hands a fragment to Defrag); this library starts with it OFF, like the ones above: Decode
 * punts fragments.  defrag_cache_max: decode-defrag.c:24, read when the table is created. */
uint32_t defrag_able = 0;
uint32_t defrag_cache_max = 8;
PluginModule plugin_modules[PLUGIN_SIZE];

struct ppe_tree_set {
    uint32_t generation;
    uint64_t token;  /* ppe_rules_stage's: published when this set's unit becomes the running one */
    ppe_acl_stats_t stats;
};
struct ppe_tree_node {
    uint32_t generation;
};

static ppe_ctx_t *g_ctx = NULL;
static uint32_t g_generation = 0;

unit_tree_t g_acltree_1, g_acltree_2;
unsigned long g_acltree_running = 0;
rwlock_t acltree_running_rwlock = PPE_RWLOCK_INITIALIZER;
static uint64_t g_published = 0;  /* the token of the classifier the engine runs (under g_ctx_lock) */
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
/* The engine context is thread-compatible, not thread-safe (include/ppe_hip.h): every call that uses g_ctx — a
 * Decode flush's classify, a rule commit, an ACL lookup, the release — holds g_ctx_lock, always the innermost lock
 * (g_lock and rulelist_mutex may be held around it, never taken inside it). */
static pthread_mutex_t g_ctx_lock = PTHREAD_MUTEX_INITIALIZER;
/* the detector's table (created by the first flush with portscan_able == 1, destroyed with the context) and the
 * clock DP_PortScan_Clock last gave; all under g_ctx_lock */
static ppe_portscan_t *g_ps = NULL;
static uint64_t g_ps_cycles = 0, g_ps_seconds = 0;
/* the context has the shim's flow table (created by the first flush with flow_able == 1, destroyed with the context)
 * and the clock DP_Flow_Clock last gave; both under g_ctx_lock */
static int g_flow = 0;
static uint64_t g_flow_now = 0;
/* the FCB table (created by the first flush with defrag_able == 1 that has a fragment, destroyed with the context),
 * the clock DP_Defrag_Clock last gave, and the registry of the mbufs the table holds: a fragment's id in the table is
 * its slot here (never ~0), free slots on a stack; all under g_ctx_lock */
static ppe_defrag_t *g_df = NULL;
static uint64_t g_df_now = 0;
/* of the table: fcb_max x cache_max (the most fragments it holds), cache_max, fcb_max, reasm_buf_bytes */
static uint32_t g_df_ids = 0, g_df_cm = 0, g_df_fcb = 0, g_df_rb = 0;
static mbuf_t **g_held = NULL;
static uint32_t *g_held_free = NULL;
static uint32_t g_held_cap = 0, g_held_nfree = 0;
/* the monitors' object (created on first use with DP_Attack_Del_All's all-zero rules, destroyed with the context), the
 * hold time its rules were last set with, and the clock DP_Attack_Clock / _Tick last gave; all under g_ctx_lock */
static ppe_attack_t *g_atk = NULL;
static uint32_t g_atk_hold = 0;
static uint64_t g_atk_now = 0;
static fw_alert fw_log_fun = NULL;
static ppe_output_fn out_fw = NULL, out_drop = NULL, out_punt = NULL;

struct ppe_ctx *ppe_compat_ctx(void) { return g_ctx; }

void reg_fw_alert(fw_alert fun) { fw_log_fun = fun; }

void DP_Log_Func(mbuf_t *m) {
    if (m && fw_log_fun) fw_log_fun((void *)m);
}

void ppe_set_output_hooks(ppe_output_fn fw, ppe_output_fn drop, ppe_output_fn punt) {
    out_fw = fw;
    out_drop = drop;
    out_punt = punt;
}

/* ---- the registry of held fragments (caller holds g_ctx_lock) ---- */
static uint64_t held_put(mbuf_t *m) {  /* the mbuf's handle, or ~0 without memory */
    if (!g_held_nfree) {
        const uint32_t cap = g_held_cap ? g_held_cap * 2u : 1024u;
        mbuf_t **h = (mbuf_t **)realloc(g_held, sizeof(*h) * cap);
        if (h) g_held = h;
        uint32_t *f = h ? (uint32_t *)realloc(g_held_free, sizeof(*f) * cap) : NULL;
        if (f) g_held_free = f;
        if (!h || !f) return ~0ull;
        for (uint32_t k = cap; k > g_held_cap; k--) {  /* (the lowest new slot on top) */
            g_held[k - 1] = NULL;
            g_held_free[g_held_nfree++] = k - 1;
        }
        g_held_cap = cap;
    }
    const uint32_t s = g_held_free[--g_held_nfree];
    g_held[s] = m;
    return s;
}

static mbuf_t *held_take(uint64_t h) {  /* the mbuf behind a handle (NULL: not one of ours), its slot free again */
    if (h >= g_held_cap || !g_held[h]) return NULL;
    mbuf_t *m = g_held[h];
    g_held[h] = NULL;
    g_held_free[g_held_nfree++] = (uint32_t)h;
    return m;
}

/* Destroy the FCB table and empty the registry: returns the mbufs it held (malloc'd array, *n entries; NULL when
 * none, or without memory for the list: then they are lost to the hooks, as a reference core that runs out of memory
 * loses them) for the caller to hand to the drop hook once no lock is held. */
static mbuf_t **defrag_reset_locked(uint32_t *n) {
    *n = 0;
    if (g_df) ppe_defrag_destroy(g_df);
    g_df = NULL;
    uint32_t live = g_held_cap - g_held_nfree;
    mbuf_t **out = live ? (mbuf_t **)malloc(sizeof(*out) * live) : NULL;
    for (uint32_t s = 0; s < g_held_cap; s++)
        if (g_held[s] && out) out[(*n)++] = g_held[s];
    free(g_held);
    free(g_held_free);
    g_held = NULL;
    g_held_free = NULL;
    g_held_cap = g_held_nfree = 0;
    return out;
}

int DP_Acl_Rule_Init(void) {
    pthread_mutex_lock(&g_lock);
    int rc = SEC_OK;
    if (!g_ctx) {
        const char *d = getenv("PPE_DEVICE");
        if (ppe_ctx_create(d ? atoi(d) : 0, &g_ctx) != PPE_OK) {
            g_ctx = NULL;
            rc = SEC_NO;
        }
    }
    if (rc == SEC_OK && !rule_list && ppe_rule_list_init() != 0) rc = SEC_NO;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

static void publish_stats(const ppe_acl_stats_t *st) {
    gWstDepth = (int)st->max_depth;
    gChildCount = (int)st->n_leaves;
    gAvgDepth = (int)(st->avg_depth * st->n_leaves + 0.5);
    gNumTreeNode = (int)st->n_nodes;
    gNumLeafNode = (int)st->n_leaves;
}

/* The classifier the running unit names (g_acltree_running, set by dp_cmd.c's set_running_acltree) becomes the
 * engine's running image at the next classify step or lookup: its token is read under the rwlock's read side (the
 * unit's handles stay valid while it is running: dp_cmd.c cleans only the back unit), then published once.
 * Caller holds g_ctx_lock. */
static void sync_running_locked(void) {
    read_lock(&acltree_running_rwlock);
    const unit_tree_t *u = (const unit_tree_t *)g_acltree_running;
    const uint64_t token = (u && u->TreeSet) ? u->TreeSet->token : 0;
    read_unlock(&acltree_running_rwlock);
    if (g_ctx && token && token != g_published && ppe_rules_publish(g_ctx, token) == PPE_OK) g_published = token;
}

uint32_t DP_Acl_Load_Rule(rule_list_t *rl, TreeSet **tset, TreeNode **tnode) {
    if (!rl) return SEC_NO;
    RCP_BLOCK_ACL_RULE_TUPLE *t = (RCP_BLOCK_ACL_RULE_TUPLE *)malloc(sizeof(*t) * RULE_ENTRY_MAX);
    uint8_t *used = (uint8_t *)malloc(RULE_ENTRY_MAX);
    if (!t || !used) {
        free(t);
        free(used);
        return SEC_NO;
    }
    for (int i = 0; i < RULE_ENTRY_MAX; i++) {
        memcpy(&t[i], &rl->rule_entry[i].rule_tuple, sizeof(*t));
        used[i] = (uint8_t)rl->rule_entry[i].entry_status;
    }
    ppe_acl_stats_t st;
    uint64_t token = 0;
    pthread_mutex_lock(&g_ctx_lock);
    /* A switch of g_acltree_running that no classify step has synced yet reaches the engine first: the engine has
     * two slots, and the stage below reuses the back one, which may hold exactly that unpublished classifier. */
    sync_running_locked();
    const int rc = g_ctx ? ppe_rules_stage(g_ctx, t, used, RULE_ENTRY_MAX, dp_acl_action_default, &st, &token)
                         : PPE_ENODEV;
    pthread_mutex_unlock(&g_ctx_lock);
    free(t);
    free(used);
    if (rc != PPE_OK) return SEC_NO;
    publish_stats(&st);
    ++g_generation;
    if (tset) {
        struct ppe_tree_set *s = (struct ppe_tree_set *)calloc(1, sizeof *s);
        if (s) {
            s->generation = g_generation;
            s->token = token;
            s->stats = st;
        }
        *tset = s;
    }
    if (tnode) {
        struct ppe_tree_node *n = (struct ppe_tree_node *)calloc(1, sizeof *n);
        if (n) n->generation = g_generation;
        *tnode = n;
    }
    return SEC_OK;
}

void DP_Acl_Rule_Clean(TreeSet **tset, TreeNode **tnode) {
    if (tset && *tset) {
        free(*tset);
        *tset = NULL;
    }
    if (tnode && *tnode) {
        free(*tnode);
        *tnode = NULL;
    }
}

void DP_Acl_Rule_Release(void) {
    pthread_mutex_lock(&g_lock);
    pthread_mutex_lock(&g_ctx_lock);  /* no flush, commit or lookup is using the context being destroyed */
    if (g_ps) ppe_portscan_destroy(g_ps);  /* (before its context) */
    g_ps = NULL;
    if (g_atk) ppe_attack_destroy(g_atk);  /* (before its context: its rules and state go with it) */
    g_atk = NULL;
    uint32_t nheld = 0;
    mbuf_t **held = defrag_reset_locked(&nheld);  /* the FCB table, and what it held for the drop hook below */
    if (g_ctx) ppe_ctx_destroy(g_ctx);  /* (its flow table with it) */
    g_ctx = NULL;
    g_flow = 0;
    g_published = 0;  /* (a new context numbers its tokens from 1 again) */
    pthread_mutex_unlock(&g_ctx_lock);
    write_lock(&acltree_running_rwlock);
    g_acltree_running = 0;
    write_unlock(&acltree_running_rwlock);
    DP_Acl_Rule_Clean(&g_acltree_1.TreeSet, &g_acltree_1.TreeNode);
    DP_Acl_Rule_Clean(&g_acltree_2.TreeSet, &g_acltree_2.TreeNode);
    pthread_mutex_unlock(&g_lock);
    for (uint32_t i = 0; i < nheld; i++)  /* (no lock held) */
        if (out_drop) out_drop(held[i]);
    free(held);
}

int DP_Acl_Rule_Commit(void) {
    if (!rule_list) return SEC_NO;
    int rc = SEC_OK;
    pthread_mutex_lock(&rule_list->rulelist_mutex);
    if (rule_list->build_status != RULE_BUILD_COMMIT) {
        /* dp_cmd.c:2017-2031: build the back tree, make it the running one, clean the new back one */
        unit_tree_t *back = g_acltree_running == (unsigned long)(void *)&g_acltree_1 ? &g_acltree_2 : &g_acltree_1;
        if (DP_Acl_Load_Rule(rule_list, &back->TreeSet, &back->TreeNode) != SEC_OK) {
            rc = SEC_NO;  /* "commit failed" */
        } else {
            write_lock(&acltree_running_rwlock);
            g_acltree_running = (unsigned long)(void *)back;
            write_unlock(&acltree_running_rwlock);
            pthread_mutex_lock(&g_ctx_lock);
            sync_running_locked();  /* (published now, not at the next batch: the commit's caller expects it) */
            pthread_mutex_unlock(&g_ctx_lock);
            unit_tree_t *old = back == &g_acltree_1 ? &g_acltree_2 : &g_acltree_1;
            DP_Acl_Rule_Clean(&old->TreeSet, &old->TreeNode);
        }
        rule_list->build_status = RULE_BUILD_COMMIT;  /* set either way, dp_cmd.c:2048 */
    }
    pthread_mutex_unlock(&rule_list->rulelist_mutex);
    return rc;
}

static void mbuf_tuple(const mbuf_t *m, uint32_t *tw, uint32_t *mw) {
    tw[0] = m->ipv4.sip;
    tw[1] = m->ipv4.dip;
    tw[2] = (uint32_t)m->sport | ((uint32_t)m->dport << 16);
    tw[3] = m->proto;
    const uint8_t *d = m->eth_dst, *s = m->eth_src;
    mw[0] = (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
    mw[1] = (uint32_t)d[4] | ((uint32_t)d[5] << 8);
    mw[2] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    mw[3] = (uint32_t)s[4] | ((uint32_t)s[5] << 8);
}

int DP_Acl_Lookup_Burst(mbuf_t **m, uint32_t n, int *actions) {
    if (!m) return PPE_EINVAL;
    if (n == 0) return PPE_OK;
    /* a short burst (DP_Acl_Lookup's one flow miss, flow.c:232) stays on the stack: no allocation per call */
    enum { kStack = 64 };
    uint32_t s_tw[4 * kStack], s_mw[4 * kStack], s_act[kStack];
    uint64_t s_ts[kStack];
    int32_t s_hit[kStack];
    const int heap = n > kStack;
    uint32_t *tw = heap ? (uint32_t *)malloc((size_t)n * 16) : s_tw, *mw = heap ? (uint32_t *)malloc((size_t)n * 16) : s_mw;
    uint64_t *ts = heap ? (uint64_t *)malloc((size_t)n * 8) : s_ts;
    int32_t *hit = heap ? (int32_t *)malloc((size_t)n * 4) : s_hit;
    uint32_t *act = heap ? (uint32_t *)malloc((size_t)n * 4) : s_act;
    int rc = PPE_ENOMEM;
    if (tw && mw && ts && hit && act) {
        for (uint32_t i = 0; i < n; i++) {
            mbuf_tuple(m[i], tw + 4 * i, mw + 4 * i);
            ts[i] = m[i]->timestamp;
        }
        ppe_tuples_t in = {tw, mw, ts, n};
        pthread_mutex_lock(&g_ctx_lock);
        sync_running_locked();
        rc = g_ctx ? ppe_acl_lookup_host(g_ctx, &in, hit, act, 0) : PPE_EINVAL;
        pthread_mutex_unlock(&g_ctx_lock);
        if (rc == PPE_OK)
            for (uint32_t i = 0; i < n; i++) {
                m[i]->ppe_acl_hit = hit[i];
                if (actions) actions[i] = act[i] == ACL_RULE_ACTION_DROP ? ACL_RULE_ACTION_DROP : ACL_RULE_ACTION_FW;
            }
    }
    if (heap) {
        free(tw);
        free(mw);
        free(ts);
        free(hit);
        free(act);
    }
    return rc;
}

int DP_Acl_Lookup(mbuf_t *m) {
    int a = ACL_RULE_ACTION_FW;
    if (!m || DP_Acl_Lookup_Burst(&m, 1, &a) != PPE_OK) return (int)dp_acl_action_default;
    return a;
}

/* ---- Decode burst ----
 * One burst per thread (the reference decodes on the core that received the packet, main.c:301).  The GPU step of a
 * flush is serialised per process (one engine context, thread-compatible); the output hooks run after it with no
 * lock held.  The header window holds every byte the reference's decoders read (Ethernet 14 + VLAN 4 + IPv4 60 +
 * TCP 60 = 138 B): no packet PUNTs for its window and every TCP option is parsed (ppe_hip.h ppe_batch_t.stride). */
#define PPE_COMPAT_STRIDE 144u
typedef struct {
    mbuf_t **m;
    uint32_t n, alloc;
} burst_t;

/* 1 (the default): Decode(m) classifies m and delivers it through a hook before it returns, the reference's contract
 * (decode.c:13-28: the packet is output or dropped inside Decode), so a mainloop linked unchanged (main.c:296-301)
 * sees every packet completed; a caller that calls Decode_Flush() opts into bursts with Decode_Set_Burst(n). */
static volatile uint32_t g_burst_cap = 1;
static pthread_key_t g_burst_key;
static pthread_once_t g_burst_once = PTHREAD_ONCE_INIT;
static __thread burst_t *t_burst = NULL;

/* Test hook (tests/test_compat_host.py only, not in the public headers): the next `k` allocations of the Decode
 * path fail, so the allocation-failure branches can be exercised without exhausting memory. */
static volatile uint32_t g_fail_alloc = 0;
void ppe_compat_debug_fail_alloc(uint32_t k) { __atomic_store_n(&g_fail_alloc, k, __ATOMIC_RELAXED); }
static int take_fail(void) {
    uint32_t k = __atomic_load_n(&g_fail_alloc, __ATOMIC_RELAXED);
    while (k)
        if (__atomic_compare_exchange_n(&g_fail_alloc, &k, k - 1, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return 1;
    return 0;
}
/* Test hook (tests/test_gpu_compat_defrag.py only, not in the public headers): the next flush with defrag_able == 1
 * that reaches step `step` fails there with PPE_EIO, once: 1 the defrag step (before ppe_defrag_host, its mbufs already
 * in the registry), 2 the datagrams' classify step.  0 disarms. */
static volatile uint32_t g_fail_step = 0;
void ppe_compat_debug_fail_defrag_step(uint32_t step) { __atomic_store_n(&g_fail_step, step, __ATOMIC_RELAXED); }
static int take_step_fail(uint32_t step) {
    uint32_t want = step;
    return __atomic_compare_exchange_n(&g_fail_step, &want, 0u, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
}
static void *burst_alloc(size_t bytes, size_t align) {
    if (take_fail()) return NULL;
    return align ? aligned_alloc(align, (bytes + align - 1) / align * align) : malloc(bytes);
}

static int flush_burst(burst_t *b);

static void burst_exit(void *p) {  /* thread exit: deliver what the thread left queued, then free its burst */
    burst_t *b = (burst_t *)p;
    if (!b) return;
    flush_burst(b);
    /* a Decode() from a later TLS destructor of this thread must start a new burst, not touch this one */
    t_burst = NULL;
    free(b->m);
    free(b);
}

static void burst_key_init(void) { pthread_key_create(&g_burst_key, burst_exit); }

static burst_t *my_burst(void) {
    if (!t_burst) {
        pthread_once(&g_burst_once, burst_key_init);
        t_burst = (burst_t *)calloc(1, sizeof(burst_t));
        if (t_burst) pthread_setspecific(g_burst_key, t_burst);
    }
    return t_burst;
}

void Decode_Set_Burst(uint32_t n) {
    if (n) __atomic_store_n(&g_burst_cap, n, __ATOMIC_RELAXED);
}

/* statuses on which the reference calls DP_Log_Func before dropping (not StreamTcp's drops, PPE_ST_STREAM_*:
 * flow.c:316-319 goes to output_drop_proc without it) */
static int logged_drop(uint32_t st) {
    switch (st) {
        case PPE_ST_L2_HEADER_ERR: case PPE_ST_VLAN_HEADER_ERR: case PPE_ST_IPV4_HEADER_ERR:
        case PPE_ST_IPV4_VERSION_ERR: case PPE_ST_IPV4_LEN_ERR: case PPE_ST_FRAG_LEN_ERR:
        case PPE_ST_UDP_HEADER_ERR: case PPE_ST_UDP_LEN_ERR: case PPE_ST_TCP_HEADER_ERR:
        case PPE_ST_TCP_LEN_ERR: case PPE_ST_ACL_DROP:
            return 1;
        default:
            return 0;
    }
}

/* The mbuf fields the reference's decoders write, exactly on the packets where they write them, from the kernel's
 * outputs for the packet (verdict, tuple) and its length.  Which layer wrote what follows from the terminal status:
 * the decoders run in order and each writes its fields once its own checks have passed.  Header pointers are the
 * packet's own addresses at the offsets the decoders use (IPV4_GET_HLEN / TCP_GET_HLEN read the same header bytes
 * the reference reads); no field is derived by re-decoding the packet here.  There is no host flow object, with or
 * without the flow table: m->flow stays as it was (FlowHandlePacket sets it to the flow item, flow.c:306).
 * flow_on: the burst went through the flow table (flow_able == 1). */
static void fill_mbuf(mbuf_t *m, uint32_t v, uint32_t fhash, int32_t hit, const uint32_t *tu, int flow_on) {
    const uint32_t st = PPE_VERDICT_STATUS(v), fl = PPE_VERDICT_FLAGS(v);
    uint8_t *pkt = (uint8_t *)m->pkt_ptr;
    m->ppe_verdict = v;
    m->ppe_flow_hash = fhash;
    m->ppe_acl_hit = hit;
    if (!pkt || st == PPE_ST_L2_HEADER_ERR) return;  /* DecodeEthernet failed before writing anything */
    /* DecodeEthernet: decode-ethernet.c:57, 71-72 */
    m->ethh = pkt;
    memcpy(m->eth_dst, pkt, 6);
    memcpy(m->eth_src, pkt + 6, 6);
    if (fl & PPE_F_VLAN) {  /* DecodeVLAN passed its checks: decode-vlan.c:41, 46 */
        m->vlanh = pkt + 14;
        m->vlan_idx = 1;
    }
    if (st == PPE_ST_L2_UNSUPPORT || st == PPE_ST_VLAN_HEADER_ERR || st == PPE_ST_VLAN_LAYER_EXCEED ||
        st == PPE_ST_VLAN_UNSUPPORT)
        return;  /* never reached DecodeIPV4 */
    /* DecodeIPV4Packet: network_header once len >= 20 and the version is 4 (decode-ipv4.c:30-42): an
     * IPV4_HEADER_ERR is either check order's first failure (len < 20) or the header length (after :42) */
    const uint32_t l3off = 14u + ((fl & PPE_F_VLAN) ? 4u : 0u);
    const uint32_t l3len = ((m->pkt_totallen & 0xffffu) - l3off) & 0xffffu;
    if (st == PPE_ST_IPV4_VERSION_ERR || (st == PPE_ST_IPV4_HEADER_ERR && l3len < 20u)) return;
    uint8_t *l3 = pkt + l3off;
    m->network_header = l3;
    if (st == PPE_ST_IPV4_HEADER_ERR || st == PPE_ST_IPV4_LEN_ERR) return;
    /* every IPv4 check passed: decode-ipv4.c:62-63, 97 */
    m->ipv4.sip = tu[0];
    m->ipv4.dip = tu[1];
    m->proto = (uint8_t)tu[3];
    if (st == PPE_ST_FRAG || st == PPE_ST_FRAG_LEN_ERR) {  /* decode-ipv4.c:106-109 (Defrag reads them) */
        m->defrag_id = (uint16_t)tu[2];
        m->frag_offset = (uint16_t)(tu[2] >> 16);
        m->frag_len = (uint16_t)(tu[3] >> 16);
        return;
    }
    const int tcp = m->proto == 6u;
    if (st == PPE_ST_IPV4_UNSUPPORT || st == PPE_ST_UDP_HEADER_ERR || st == PPE_ST_TCP_HEADER_ERR) return;
    /* the UDP-flood monitor sits ahead of DecodeUDP (decode-ipv4.c:141-149): nothing of layer 4 is written.  The TCP
     * monitors sit behind DecodeTCP's length checks (decode-tcp.c:146, 162-173): transport_header, then the return below
     * (a monitor drop has no PPE_F_L4), so ports 0, no PKT_HAS_FLOW, no direction flag */
    if (st == PPE_ST_ATTACK_UDPFLOOD) return;
    /* the L4 decoder's first length check passed: decode-udp.c:24, decode-tcp.c:146 */
    uint8_t *l4 = l3 + (l3[0] & 0x0fu) * 4u;
    m->transport_header = l4;
    if (!(fl & PPE_F_L4)) return;  /* UDP_LEN_ERR / TCP_LEN_ERR */
    /* decode-udp.c:38-45, decode-tcp.c:175-187 */
    m->sport = (uint16_t)tu[2];
    m->dport = (uint16_t)(tu[2] >> 16);
    m->payload_len = (uint16_t)(tu[3] >> 16);
    m->payload = l4 + (tcp ? (uint32_t)(l4[12] >> 4) * 4u : 8u);
    const uint32_t ws = PPE_TUPLE_WS(tu[3]);
    if (tcp && ws && !m->tcpvars.ws) {  /* DecodeTCPOptions' window-scale record (decode-tcp.c:61-70), found by the
                                          * kernel; like the reference, only into an mbuf with none recorded yet */
        uint8_t *o = l4 + ws;
        m->tcpvars.tcp_opts[0].type = o[0];
        m->tcpvars.tcp_opts[0].len = o[1];
        m->tcpvars.tcp_opts[0].data = o + 2;
        m->tcpvars.ws = &m->tcpvars.tcp_opts[0];
    }
    /* FlowHandlePacket found or created the flow (ACL passed): flow.c:294-307.  Every packet of the stateless path
     * is its flow's first, and FlowAdd orients the flow as that packet, so the direction is to-server.
     * StreamTcp runs after that (flow.c:311-320), so a packet it drops carries the flags too.  A packet the port-scan
     * detector dropped has no flow: FlowGetFlowFromHash returned NULL before FlowAdd (flow.c:216-230). */
    if (flow_on) {
        /* the flow table: the kernel's own flags (flow.c:248-307): a found or created flow, its direction against the
         * packet that created it; a FLOW_NOMEM, NO_SYN_FIRST or ACL-dropped packet has no flow and carries neither */
        if (fl & PPE_F_FLOW) m->flags |= PKT_HAS_FLOW | ((fl & PPE_F_TOCLIENT) ? PKT_TO_CLIENT : PKT_TO_SERVER);
        return;
    }
    if (st == PPE_ST_ACL_FW || (st >= PPE_ST_STREAM_RST_NO_SESSION && st <= PPE_ST_STREAM_MIDSTREAM_OFF))
        m->flags |= PKT_TO_SERVER | PKT_HAS_FLOW;
}

/* FlowInit behind Decode, caller holds g_ctx_lock and g_ctx is set: the table on first use (flow_item_num flows;
 * max_batch at least this burst: a later, larger burst goes through it in chunks). */
static int flow_prepare_locked(uint32_t n) {
    if (g_flow) return PPE_OK;
    const int rc = ppe_flow_create(g_ctx, flow_item_num, ((n > 4096u ? n : 4096u) + 63u) & ~63u);
    if (rc == PPE_OK) g_flow = 1;
    return rc;
}

void DP_Flow_Clock(uint64_t now_seconds) {
    pthread_mutex_lock(&g_ctx_lock);
    g_flow_now = now_seconds;
    pthread_mutex_unlock(&g_ctx_lock);
}

int DP_Flow_Age(uint64_t now_seconds, uint64_t *deleted) {
    if (deleted) *deleted = 0;
    pthread_mutex_lock(&g_ctx_lock);
    const int rc = (g_ctx && g_flow) ? ppe_flow_age(g_ctx, now_seconds, 20u /* FLOW_MAX_TIMEOUT */, deleted) : PPE_OK;
    pthread_mutex_unlock(&g_ctx_lock);
    return rc;
}

/* PortScan_Detect behind Decode (flow.c:215-230), caller holds g_ctx_lock and g_ctx is set: the table on first use
 * (PORTSCAN_ITEM_NUM records; max_batch at least this burst: a later, larger burst goes through it in chunks), then
 * the globals and the clock by value for this burst, attached: to the stateless path (portscan_able), or with flow_point
 * to the flow table's (flow_portscan_able, the detector on flow misses). */
static int portscan_prepare_locked(uint32_t n, int flow_point) {
    if (!g_ps) {
        ppe_portscan_cfg_t c = {1u, 0u, 50u, 600u, 100000u, 0u, 1000000000ull, 0u};
        c.max_batch = ((n > 4096u ? n : 4096u) + 63u) & ~63u;
        const int rc = ppe_portscan_create(g_ctx, &c, &g_ps);
        if (rc != PPE_OK) {
            g_ps = NULL;
            return rc;
        }
    }
    ppe_portscan_cfg_t v = {1u, portscan_action ? 1u : 0u, portscan_exception_freq, flood_hold_time, 0u, 0u, 0u, 0u};
    int rc = ppe_portscan_set(g_ps, &v);
    if (rc == PPE_OK) rc = ppe_portscan_clock(g_ps, g_ps_cycles, g_ps_seconds);
    /* a table sits on one of the two attachment points: off the other first */
    if (rc == PPE_OK) rc = flow_point ? ppe_portscan_attach(g_ctx, NULL) : ppe_flow_portscan_attach(g_ctx, NULL);
    if (rc == PPE_OK) rc = flow_point ? ppe_flow_portscan_attach(g_ctx, g_ps) : ppe_portscan_attach(g_ctx, g_ps);
    return rc;
}

void DP_PortScan_Clock(uint64_t now_cycles, uint64_t now_seconds) {
    pthread_mutex_lock(&g_ctx_lock);
    g_ps_cycles = now_cycles;
    g_ps_seconds = now_seconds;
    pthread_mutex_unlock(&g_ctx_lock);
}

int DP_PortScan_Age(uint64_t now_cycles, uint64_t *freed) {
    if (freed) *freed = 0;
    pthread_mutex_lock(&g_ctx_lock);
    const int rc = g_ps ? ppe_portscan_age(g_ps, now_cycles, freed) : PPE_OK;
    pthread_mutex_unlock(&g_ctx_lock);
    return rc;
}

ppe_portscan_t *DP_PortScan_Table(void) {
    pthread_mutex_lock(&g_ctx_lock);
    ppe_portscan_t *t = g_ps;
    pthread_mutex_unlock(&g_ctx_lock);
    return t;
}

/* ---- the monitors behind Decode (ppe_decode.h) ---- */
/* caller holds g_ctx_lock and g_ctx is set: the object on first use (all-zero rules, DP_Attack_Del_All's state), then
 * flood_hold_time as it is now (the rules in force kept) */
static int attack_object_locked(void) {
    if (!g_atk) {
        ppe_attack_cfg_t c;
        memset(&c, 0, sizeof c);
        c.hold_seconds = flood_hold_time;
        int rc = ppe_attack_create(g_ctx, &c, &g_atk);
        if (rc != PPE_OK) {
            g_atk = NULL;
            return rc;
        }
        g_atk_hold = c.hold_seconds;
        rc = ppe_attack_clock(g_atk, g_atk_now);
        if (rc != PPE_OK) return rc;
    }
    if (g_atk_hold != flood_hold_time) {  /* dp_attack_defend_time_set: read per flush, as the detector path reads it */
        ppe_attack_info_t *fi = (ppe_attack_info_t *)malloc(sizeof *fi);
        if (!fi) return PPE_ENOMEM;
        int rc = ppe_attack_info(g_atk, fi);
        if (rc == PPE_OK) {
            fi->cfg.hold_seconds = flood_hold_time;
            rc = ppe_attack_set(g_atk, &fi->cfg);
        }
        if (rc == PPE_OK) g_atk_hold = fi->cfg.hold_seconds;
        free(fi);
        return rc;
    }
    return PPE_OK;
}

ppe_attack_t *DP_Attack_Object(void) {
    pthread_mutex_lock(&g_ctx_lock);
    if (g_ctx && !g_atk) (void)attack_object_locked();
    ppe_attack_t *t = g_atk;
    pthread_mutex_unlock(&g_ctx_lock);
    return t;
}

int DP_Attack_Rule_Set(const ppe_attack_cfg_t *cfg) {
    if (!cfg) return PPE_EINVAL;
    pthread_mutex_lock(&g_ctx_lock);
    int rc = g_ctx ? attack_object_locked() : PPE_ENODEV;
    if (rc == PPE_OK) {
        ppe_attack_cfg_t c = *cfg;
        c.hold_seconds = flood_hold_time;  /* (the shim's hold time is the global's, not the argument's) */
        c.pad = 0;
        rc = ppe_attack_set(g_atk, &c);
        if (rc == PPE_OK) g_atk_hold = c.hold_seconds;
    }
    pthread_mutex_unlock(&g_ctx_lock);
    return rc;
}

void DP_Attack_Del_All(void) {
    ppe_attack_cfg_t c;
    memset(&c, 0, sizeof c);
    pthread_mutex_lock(&g_ctx_lock);
    if (g_atk) {  /* (no object: its rules are all zero when it is created) */
        c.hold_seconds = flood_hold_time;
        if (ppe_attack_set(g_atk, &c) == PPE_OK) g_atk_hold = c.hold_seconds;
    }
    pthread_mutex_unlock(&g_ctx_lock);
}

void DP_Attack_Clock(uint64_t now_seconds) {
    pthread_mutex_lock(&g_ctx_lock);
    g_atk_now = now_seconds;
    if (g_atk) (void)ppe_attack_clock(g_atk, now_seconds);
    pthread_mutex_unlock(&g_ctx_lock);
}

int DP_Attack_Tick(uint64_t now_seconds) {
    pthread_mutex_lock(&g_ctx_lock);
    g_atk_now = now_seconds;
    const int rc = g_atk ? ppe_attack_tick(g_atk, now_seconds) : PPE_OK;  /* (no object: nothing counted yet) */
    pthread_mutex_unlock(&g_ctx_lock);
    return rc;
}

/* Classify `n` mbufs on the GPU (serialised) and fill their parse fields; returns PPE_OK or a PPE_E* code. */
static int classify_mbufs(mbuf_t **mb, uint32_t n) {
    uint8_t *hdr = (uint8_t *)burst_alloc((size_t)n * PPE_COMPAT_STRIDE, 16);
    uint8_t *port = (uint8_t *)burst_alloc((size_t)n, 0);
    uint32_t *len = (uint32_t *)burst_alloc((size_t)n * 4, 0), *verdict = (uint32_t *)burst_alloc((size_t)n * 4, 0);
    uint32_t *fh = (uint32_t *)burst_alloc((size_t)n * 4, 0), *tuple = (uint32_t *)burst_alloc((size_t)n * 16, 0);
    uint64_t *ts = (uint64_t *)burst_alloc((size_t)n * 8, 0);
    int32_t *hit = (int32_t *)burst_alloc((size_t)n * 4, 0);
    int rc = PPE_ENOMEM;
    if (hdr && len && verdict && fh && tuple && ts && hit && port) {
        memset(hdr, 0, (size_t)n * PPE_COMPAT_STRIDE);
        for (uint32_t i = 0; i < n; i++) {
            mbuf_t *m = mb[i];
            const uint32_t c = m->pkt_totallen < PPE_COMPAT_STRIDE ? m->pkt_totallen : PPE_COMPAT_STRIDE;
            if (m->pkt_ptr && c) memcpy(hdr + (size_t)i * PPE_COMPAT_STRIDE, m->pkt_ptr, c);
            len[i] = m->pkt_totallen;
            ts[i] = m->timestamp;
            port[i] = (uint8_t)m->input_port;  /* (a reassembled datagram: its chain head's, defrag_mbufs) */
        }
        ppe_batch_t b = {hdr, len, ts, n, PPE_COMPAT_STRIDE};
        ppe_result_t r;
        memset(&r, 0, sizeof r);
        r.verdict = verdict;
        r.flow_hash = fh;
        r.acl_hit = hit;
        r.tuple = tuple;
        ppe_cfg_t cfg = {unsupport_proto_action ? 1u : 0u, syn_check ? 1u : 0u, 0};
        const ppe_stream_tcp_cfg_t stcp = {stream_tcp_track_enable ? 1u : 0u, stream_tcp_midstream ? 1u : 0u,
                                           stream_tcp_async_oneside ? 1u : 0u, 0u};
        const int flow_on = flow_able == 1u;  /* (any other value is off) */
        pthread_mutex_lock(&g_ctx_lock);
        sync_running_locked();
        if (flow_on) cfg.now_seconds = g_flow_now;  /* FLOW_UPDATE_TIMESTAMP's clock */
        if (g_ctx && flow_on && (portscan_able == 1u || stream_tcp_track_enable)) {
            /* portscan_able is the stateless path's switch (the flow table's detector is flow_portscan_able) and the TCP
             * session machine is not built: the burst is refused before any state changes (ppe_decode.h) */
            rc = PPE_ENOTSUP;
        } else {
            rc = g_ctx ? ppe_stream_tcp_set(g_ctx, &stcp) : PPE_ENODEV;
        }
        if (rc == PPE_OK && portscan_able == 1u) {  /* (dp_portscan.c:238: any other value is off) */
            rc = portscan_prepare_locked(n, 0);
            if (rc == PPE_OK) rc = ppe_classify_host_ordered(g_ctx, &b, &r, &cfg, 0);
        } else if (rc == PPE_OK) {
            const int fps_on = flow_on && flow_portscan_able == 1u;  /* (without the flow table: no effect) */
            if (g_ps) rc = ppe_portscan_attach(g_ctx, NULL);  /* the table keeps its records while off */
            if (rc == PPE_OK && g_ps && !fps_on) rc = ppe_flow_portscan_attach(g_ctx, NULL);
            const int fatk_on = flow_on && flow_attack_able == 1u;  /* (without the flow table: no effect) */
            if (rc == PPE_OK && g_atk && !fatk_on) rc = ppe_flow_attack_attach(g_ctx, NULL);  /* it keeps its state */
            if (rc == PPE_OK && flow_on) {  /* FlowHandlePacket: the table on first use, the burst in order through it */
                rc = flow_prepare_locked(n);
                if (rc == PPE_OK && fps_on) rc = portscan_prepare_locked(n, 1);  /* PortScan_Detect on its misses */
                if (rc == PPE_OK && fatk_on) {  /* the monitors ahead of the table (decode-ipv4.c:141-149, decode-tcp.c:162-173) */
                    rc = attack_object_locked();
                    if (rc == PPE_OK) rc = ppe_flow_attack_attach(g_ctx, g_atk);
                    /* with the detector as well the burst runs the combined path; the switch then stays on for the context */
                    if (rc == PPE_OK && fps_on) rc = ppe_flow_combine(g_ctx, 1u);
                }
                if (rc == PPE_OK) rc = ppe_classify_flow_host_ports(g_ctx, &b, &r, &cfg, 0, port);
            } else if (rc == PPE_OK) {
                rc = ppe_classify_host(g_ctx, &b, &r, &cfg, 0);
            }
        }
        pthread_mutex_unlock(&g_ctx_lock);
        if (rc == PPE_OK)
            for (uint32_t i = 0; i < n; i++) fill_mbuf(mb[i], verdict[i], fh[i], hit[i], tuple + 4 * (size_t)i, flow_on);
    }
    free(hdr);
    free(port);
    free(len);
    free(verdict);
    free(fh);
    free(tuple);
    free(ts);
    free(hit);
    return rc;
}

/* ---- Defrag behind Decode (decode-ipv4.c:102-125; ppe_decode.h) ---- */
void DP_Defrag_Clock(uint64_t now_seconds) {
    pthread_mutex_lock(&g_ctx_lock);
    g_df_now = now_seconds;
    pthread_mutex_unlock(&g_ctx_lock);
}

ppe_defrag_t *DP_Defrag_Table(void) {
    pthread_mutex_lock(&g_ctx_lock);
    ppe_defrag_t *t = g_df;
    pthread_mutex_unlock(&g_ctx_lock);
    return t;
}

int DP_Defrag_Age(uint64_t now_seconds, uint64_t *dropped) {
    if (dropped) *dropped = 0;
    pthread_mutex_lock(&g_ctx_lock);
    if (!g_df) {
        pthread_mutex_unlock(&g_ctx_lock);
        return PPE_OK;
    }
    const uint32_t cap = g_df_ids ? g_df_ids : 1u;
    uint64_t *ids = (uint64_t *)malloc(sizeof(*ids) * cap);
    mbuf_t **mb = (mbuf_t **)malloc(sizeof(*mb) * cap);
    uint32_t nd = 0, k = 0;
    int rc = (ids && mb) ? ppe_defrag_age(g_df, now_seconds, 20u /* FRAG_MAX_TIMEOUT */, ids, g_df_ids, &nd, NULL)
                         : PPE_ENOMEM;
    if (rc == PPE_OK)
        for (uint32_t i = 0; i < nd && i < g_df_ids; i++) {
            mbuf_t *m = held_take(ids[i]);
            if (m) mb[k++] = m;
        }
    pthread_mutex_unlock(&g_ctx_lock);
    for (uint32_t i = 0; i < k; i++)  /* Frag_defrag_timeout: output_drop_proc per held fragment, no log (:538-544) */
        if (out_drop) out_drop(mb[i]);
    if (dropped) *dropped = k;
    free(ids);
    free(mb);
    return rc;
}

/* what a flush with defrag_able == 1 does with mbuf i of the burst */
enum { DF_BY_VERDICT = 0, DF_HELD, DF_DROP, DF_DROP_LOG, DF_DGRAM,
       DF_CHAIN /* (after a failed step) on a chain this burst completed: dropped with the burst */,
       DF_GONE /* (after a failed step) delivered elsewhere meanwhile */ };
typedef struct {
    uint8_t *disp;      /* n: DF_* */
    uint32_t *dgram;    /* n: the datagram index of a DF_DGRAM mbuf */
    mbuf_t *rm;         /* nd reassembled mbufs, classified */
    uint8_t *frames;    /* their frames (rm[j].pkt_ptr points into it) */
    uint32_t nd;
    mbuf_t **lost;      /* after a failure: what the table held besides this burst's mbufs, for the drop hook */
    uint32_t nlost;
} df_step_t;

static void df_step_free(df_step_t *d) {
    free(d->disp);
    free(d->dgram);
    free(d->rm);
    free(d->frames);
    free(d->lost);
}

/* The fragments of a classified burst (status PPE_ST_FRAG) through the FCB table in burst order, then the datagrams
 * they complete through the classify step as a second burst.  PPE_OK with d filled (d->disp NULL: the burst has no
 * fragment), or a PPE_E* code: then the table is gone and d->lost holds what it held. */
static int defrag_mbufs(mbuf_t **mb, uint32_t n, df_step_t *d) {
    uint32_t nf = 0;
    size_t bytes = 0;
    for (uint32_t i = 0; i < n; i++)
        if (PPE_VERDICT_STATUS(mb[i]->ppe_verdict) == PPE_ST_FRAG && mb[i]->pkt_ptr) {
            nf++;
            bytes += ((size_t)(mb[i]->pkt_totallen < 4096u ? mb[i]->pkt_totallen : 4096u) + 3u) & ~(size_t)3;
        }
    if (!nf) return PPE_OK;
    const uint32_t ws = 128u;
    d->disp = (uint8_t *)burst_alloc(n, 0);
    d->dgram = (uint32_t *)burst_alloc((size_t)n * 4, 0);
    uint32_t *at = (uint32_t *)burst_alloc((size_t)nf * 4, 0);          /* fragment k's index in the burst */
    uint8_t *pkt = (uint8_t *)burst_alloc(bytes + 64, 0);
    uint64_t *off = (uint64_t *)burst_alloc((size_t)nf * 8, 0), *id = (uint64_t *)burst_alloc((size_t)nf * 8, 0);
    uint32_t *len = (uint32_t *)burst_alloc((size_t)nf * 4, 0), *st = (uint32_t *)burst_alloc((size_t)nf * 4, 0);
    uint32_t *of = (uint32_t *)burst_alloc((size_t)nf * 4, 0), *dlen = (uint32_t *)burst_alloc((size_t)nf * 4, 0);
    uint8_t *win = (uint8_t *)burst_alloc((size_t)nf * ws, 0);
    uint64_t *chain = NULL;
    mbuf_t **rmp = NULL;
    uint32_t cm = 0, rb = 0, nd = 0, put = 0;
    int rc = PPE_ENOMEM;
    pthread_mutex_lock(&g_ctx_lock);
    if (d->disp && d->dgram && at && pkt && off && id && len && st && of && dlen && win) {
        rc = g_ctx ? PPE_OK : PPE_ENODEV;
        if (rc == PPE_OK && !g_df) {  /* FragModule_init on first use: DEFRAG_FCB_MAX FCBs, defrag_cache_max fragments each */
            ppe_defrag_cfg_t c = {1024u, defrag_cache_max, 0u, 0u, ((n > 4096u ? n : 4096u) + 63u) & ~63u, 0u};
            rc = ppe_defrag_create(g_ctx, &c, &g_df);
            if (rc != PPE_OK) g_df = NULL;
            ppe_defrag_info_t fi;
            if (rc == PPE_OK) rc = ppe_defrag_info(g_df, &fi);
            if (rc == PPE_OK) {
                g_df_ids = fi.fcb_max * fi.cache_max;
                g_df_cm = fi.cache_max;
                g_df_fcb = fi.fcb_max;
                g_df_rb = fi.reasm_buf_bytes;
            }
        }
        if (rc == PPE_OK) {
            cm = g_df_cm;  /* (of the table, whatever the global says now) */
            rb = g_df_rb;  /* ppe_defrag_host writes datagram j's frame at j x the table's reasm_buf_bytes */
            chain = (uint64_t *)burst_alloc((size_t)nf * cm * 8, 0);
            /* a call completes at most one datagram per fragment and per FCB record (none is freed inside a call) */
            d->frames = (uint8_t *)burst_alloc((size_t)(nf < g_df_fcb ? nf : g_df_fcb) * rb, 0);
            if (!chain || !d->frames) rc = PPE_ENOMEM;
        }
        size_t o = 0;
        for (uint32_t i = 0, k = 0; rc == PPE_OK && i < n; i++) {
            mbuf_t *m = mb[i];
            d->disp[i] = DF_BY_VERDICT;
            if (PPE_VERDICT_STATUS(m->ppe_verdict) != PPE_ST_FRAG || !m->pkt_ptr) continue;
            const uint32_t c = m->pkt_totallen < 4096u ? m->pkt_totallen : 4096u;  /* (frag_buf_bytes <= 4096) */
            memcpy(pkt + o, m->pkt_ptr, c);
            off[k] = o;
            len[k] = m->pkt_totallen;
            id[k] = held_put(m);
            if (id[k] == ~0ull) rc = PPE_ENOMEM;
            else put = k + 1;
            at[k++] = i;
            o += ((size_t)c + 3u) & ~(size_t)3;
        }
        if (rc == PPE_OK && take_step_fail(1u)) rc = PPE_EIO;
        if (rc == PPE_OK) {
            const ppe_frag_batch_t in = {pkt, off, len, id, nf, 0u, g_df_now};
            const ppe_defrag_out_t out = {st, of, win, dlen, d->frames, chain, &nd, ws, 0u};
            rc = ppe_defrag_host(g_df, &in, &out, 0);
        }
        if (rc == PPE_OK) {
            d->rm = nd ? (mbuf_t *)burst_alloc(sizeof(mbuf_t) * nd, 0) : NULL;
            rmp = nd ? (mbuf_t **)burst_alloc(sizeof(mbuf_t *) * nd, 0) : NULL;
            if (nd && (!d->rm || !rmp)) rc = PPE_ENOMEM;
        }
        for (uint32_t k = 0; rc == PPE_OK && k < nf; k++) {
            const uint32_t i = at[k], s = st[k] & 0xffu;
            switch (s) {
                case PPE_DF_CACHED: case PPE_DF_SETUP_ERR:  /* cached: no hook (decode-defrag.c:391-392, 281-283) */
                    d->disp[i] = DF_HELD;
                    break;
                case PPE_DF_REASM: {
                    /* the reassembled mbuf as Frag_defrag_setup / _reasm leave it (:164-220, 241-276) */
                    const uint32_t j = of[k];
                    mbuf_t *r = &d->rm[j], *prev = NULL;
                    memset(r, 0, sizeof *r);
                    r->pkt_space = PKTBUF_SW;
                    r->magic_flag = MBUF_MAGIC_NUM;
                    r->pkt_ptr = d->frames + (size_t)j * rb;
                    r->pkt_totallen = dlen[j];
                    r->flags = PKT_FRAG_REASM_COMP;
                    for (uint32_t p = 0; p < cm && chain[(size_t)j * cm + p] != ~0ull; p++) {
                        mbuf_t *f = held_take(chain[(size_t)j * cm + p]);
                        if (!f) continue;
                        if (prev) prev->next = f;
                        else {
                            r->fragments = f;
                            r->input_port = f->input_port;
                        }
                        f->next = NULL;
                        prev = f;
                    }
                    rmp[j] = r;
                    d->disp[i] = DF_DGRAM;
                    d->dgram[i] = j;
                    break;
                }
                case PPE_DF_NOT_FRAG:  /* (the two parsers agree on what a fragment is: not reached) as without Defrag */
                    held_take(id[k]);
                    break;
                default:  /* FCB_FULL, HW2SW_ERR, DELETED, CACHE_FULL, DEFRAG_ERR: output_drop_proc */
                    held_take(id[k]);
                    d->disp[i] = s == PPE_DF_CACHE_FULL ? DF_DROP_LOG : DF_DROP;
                    break;
            }
        }
        if (rc == PPE_OK) d->nd = nd;
    }
    if (rc != PPE_OK) {
        /* this burst's mbufs leave the registry (the caller drops them with the rest of the burst); everything else
         * the table held goes with the table */
        for (uint32_t k = 0; k < put; k++) held_take(id[k]);
        if (g_df || g_held_cap) d->lost = defrag_reset_locked(&d->nlost);
    }
    pthread_mutex_unlock(&g_ctx_lock);
    /* the datagrams: a second burst behind the first, in the order of their completing fragments, on the same path */
    if (rc == PPE_OK && nd) {
        rc = take_step_fail(2u) ? PPE_EIO : classify_mbufs(rmp, nd);
        if (rc != PPE_OK) {
            /* The chains' members are out of the registry already (the REASM loop took them).  Those of this burst are
             * marked: the caller drops them with the rest of the burst, once, whatever they were before the chain took
             * them (a fragment cached earlier in this burst, or the completing one).  Those of earlier bursts are in
             * neither the registry nor this burst any more: they join what the table held. */
            mbuf_t **outside = (mbuf_t **)malloc(sizeof(*outside) * ((size_t)nd * cm + 1u));
            uint32_t nout = 0;
            for (uint32_t j = 0; j < nd; j++)
                for (mbuf_t *f = d->rm[j].fragments; f; f = f->next) {
                    uint32_t i = 0;
                    while (i < n && mb[i] != f) i++;
                    if (i < n) d->disp[i] = DF_CHAIN;
                    else if (outside) outside[nout++] = f;
                }
            pthread_mutex_lock(&g_ctx_lock);
            /* this burst's fragments that are still cached leave the registry before it is emptied: dropped with the
             * burst too.  (The lock was free during the classify step: a cached fragment that another thread's flush or
             * aging took meanwhile went to a hook there, and is not dropped here again.) */
            for (uint32_t k = 0; k < nf; k++)
                if (d->disp[at[k]] == DF_HELD) {
                    if (id[k] < g_held_cap && g_held[id[k]] == mb[at[k]]) held_take(id[k]);
                    else d->disp[at[k]] = DF_GONE;
                }
            d->lost = defrag_reset_locked(&d->nlost);
            pthread_mutex_unlock(&g_ctx_lock);
            mbuf_t **all = (mbuf_t **)realloc(d->lost, sizeof(*all) * ((size_t)d->nlost + nout + 1u));
            if (all) {
                d->lost = all;
                for (uint32_t k = 0; k < nout; k++) d->lost[d->nlost++] = outside[k];
            }
            free(outside);
        }
    }
    free(at);
    free(pkt);
    free(off);
    free(id);
    free(len);
    free(st);
    free(of);
    free(dlen);
    free(win);
    free(chain);
    free(rmp);
    return rc;
}

/* Take the burst's mbufs out (the burst is empty and reusable before any hook runs), classify, deliver.  The queued
 * array itself is taken, so a flush allocates nothing of its own: when the classify step cannot run (no context,
 * no memory, a GPU error), every taken mbuf still reaches the drop hook (decode.c:24-27; ppe_decode.h). */
static int flush_burst(burst_t *b) {
    const uint32_t n = b->n, alloc = b->alloc;
    if (n == 0) return 0;
    mbuf_t **mb = b->m;
    b->m = NULL;
    b->n = b->alloc = 0;
    int rc = classify_mbufs(mb, n);
    df_step_t df;
    memset(&df, 0, sizeof df);
    if (rc == PPE_OK && defrag_able == 1u) rc = defrag_mbufs(mb, n, &df);  /* (any other value is off) */
    uint32_t calls = 0;
    for (uint32_t i = 0; i < n; i++) {
        mbuf_t *m = mb[i];
        const uint8_t disp = (df.disp && (rc == PPE_OK || df.nd)) ? df.disp[i] : (uint8_t)DF_BY_VERDICT;
        if (rc != PPE_OK) {  /* undelivered: every packet ends in output_drop_proc (decode.c:24-27) */
            if (disp != DF_GONE && out_drop) out_drop(m);
            continue;
        }
        if (disp == DF_HELD) continue;  /* cached in its FCB: a later flush, DP_Defrag_Age or the release delivers it */
        calls++;
        if (disp == DF_DROP || disp == DF_DROP_LOG) {
            if (disp == DF_DROP_LOG) DP_Log_Func(m);  /* cache full (decode-defrag.c:436) */
            if (out_drop) out_drop(m);
            continue;
        }
        if (disp == DF_DGRAM) m = &df.rm[df.dgram[i]];  /* the datagram takes its completing fragment's place */
        const uint32_t v = m->ppe_verdict;
        switch (PPE_VERDICT_ACTION(v)) {
            case PPE_ACT_FW:
                if (out_fw) out_fw(m);
                break;
            case PPE_ACT_DROP:
                if (logged_drop(PPE_VERDICT_STATUS(v))) DP_Log_Func(m);
                if (out_drop) out_drop(m);
                break;
            default:
                if (out_punt) out_punt(m);
                break;
        }
    }
    for (uint32_t i = 0; i < df.nlost; i++)  /* a failed defrag step: what its table held (ppe_decode.h) */
        if (out_drop) out_drop(df.lost[i]);
    df_step_free(&df);
    if (b == t_burst && !b->m) {  /* no hook queued anything meanwhile: the array goes back to the burst */
        b->m = mb;
        b->alloc = alloc;
    } else {
        free(mb);
    }
    return rc == PPE_OK ? (int)calls : rc;
}

int Decode_Flush(void) {
    burst_t *b = t_burst;
    return b ? flush_burst(b) : 0;
}

void Decode(mbuf_t *m) {
    if (!m) return;
    burst_t *b = my_burst();
    const uint32_t cap = __atomic_load_n(&g_burst_cap, __ATOMIC_RELAXED);
    if (b && b->n >= b->alloc) {  /* grow to the current cap (or one more slot when the cap was lowered) */
        const uint32_t want = cap > b->n ? cap : b->n + 1;
        mbuf_t **nb = take_fail() ? NULL : (mbuf_t **)realloc(b->m, sizeof(mbuf_t *) * want);
        if (nb) {
            b->m = nb;
            b->alloc = want;
        }
    }
    if (!b || b->n >= b->alloc) {  /* no memory for the burst slot */
        if (out_drop) out_drop(m);
        return;
    }
    b->m[b->n++] = m;
    if (b->n >= cap) flush_burst(b);
}
