/*
 * ppe_engine.hip — host runtime behind the C ABI in include/ppe_hip.h.
 *
 * Owns, per context (one per GPU, like one per-core dataplane instance):
 *   - the double-buffered classifier image (g_acltree_1/2 + running pointer + rwlock-protected swap of
 *     dataplane/src/common/dp_cmd.c:1963-1985): commit writes the back image only after the last launch that
 *     read it has completed (HIP event), then flips `running` — the swap happens at a batch boundary;
 *   - per-workgroup counter slots (the per-core pktstat[] of dataplane/src/decode/decode-statistic.c:4-22);
 *   - HIP-event kernel timing, and the pipelined host-buffer path (H2D → classify → D2H on 3 streams).
 */
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ppe_hip.h"
#include "ppe_image.h"
#include "ppe_internal.h"

namespace {

constexpr int kSlotSets = 4;      // set 0: ppe_classify; 1..3: host pipeline streams
constexpr int kHostStreams = 3;
// ppe_classify_batches: two streams, so a batch's launch ramp-up overlaps the previous batch's tail (C1: 20.6 ->
// 16.5 us per batch; three streams measured 17.0)
constexpr int kPipeStreams = 2;
constexpr uint32_t kMaxBlocksPerCU = 32;  // > resident: the grid then runs in rounds (non-persistent)
// ppe_classify_batches: batches per launch.  0 = every batch of the call in one persistent launch (descriptor ring in
// device memory): the launch ramp and tail are paid once per call instead of once per batch
constexpr uint32_t kBatchesPerLaunch = 0;

struct HostStage {
    hipStream_t s = nullptr;
    uint8_t *hdr = nullptr;
    uint32_t *len = nullptr;
    uint64_t *ts = nullptr;
    uint32_t *verdict = nullptr, *fhash = nullptr, *fw = nullptr, *drop = nullptr, *tcnt = nullptr,
             *tuple = nullptr;
    int32_t *hit = nullptr;
    uint8_t *ports = nullptr;  // ppe_classify_flow_host_ports: the chunk's input-port bytes
    uint32_t cap = 0, stride = 0;
};

// Per-context staging of the host-pointer ACL lookup (DP_Acl_Lookup, one call per flow miss on the reference's hot
// path, flow.c:232): pinned, device-mapped host memory the lookup kernel reads its tuples from and writes its results
// to across PCIe (no hipMalloc, no copies, no device-wide synchronisation per call), its own stream and a spin wait
// on that stream only.
struct LookupStage {
    hipStream_t s = nullptr;
    uint8_t *h = nullptr;   // host view: tuples (16 B) | macs (16 B) | ts (8 B) | hit (4 B) | action (4 B), per entry
    uint8_t *d = nullptr;   // the same memory as the device sees it
    uint32_t cap = 0;       // entries
};

// Device flow table (ppe_classify_flow) and what the host knows about it without synchronising.
struct FlowArrays {
    uint32_t *keys = nullptr, *creator = nullptr;
    unsigned long long *stats = nullptr, *recs = nullptr;
    uint32_t *sess = nullptr;  // the TCP session records, PPE_FLOW_SESS_WORDS per slot (ppe_flow_stream_attach; else NULL)
};
struct FlowTable {
    uint32_t capacity = 0, max_batch = 0, nslots = 0;
    FlowArrays arr[2];  // arr[cur] in use; the other is the rehash target (allocated on first rehash)
    int cur = 0;
    unsigned long long *ctl = nullptr;
    uint32_t *rec = nullptr, *rslot = nullptr, *miss_tiles = nullptr;
    unsigned long long *tile_miss = nullptr, *tile_new = nullptr;
    // owner-computed FlowUpdate (flow_update_wg in ppe_flow_post_kernel): bucket columns for upd_wgs classify workgroups
    unsigned long long *upd = nullptr;
    uint32_t *ucnt = nullptr;
    uint32_t upd_wgs = 0, upd_osh = 0, upd_owners = 0, upd_hmask = PPE_UPD_HASH - 1u;
    uint64_t batches = 0;   // ppe_classify_flow calls (the parity selects the miss-tile counter)
    unsigned long long fold_pkts = PPE_PK_FOLD_PKTS, fold_bytes = PPE_PK_FOLD_BYTES;
    uint64_t live_ub = 0;   // upper bound of live flows: a snapshot's count + n per batch since
    uint64_t tomb_ub = 0;   // upper bound of tombstones: a snapshot's count + n per batch that could revoke
    uint32_t rehashes = 0;
    // zero-copy snapshot of ctl in pinned host memory, written by every flow-mode classify launch (block 0) as it
    // starts: {batches completed, live, tombstones}.  The host tightens its bounds from it without synchronising.
    // refreshes them without synchronising
    unsigned long long *snap_h = nullptr, *snap_d = nullptr;  // host / device views
    uint64_t snap_used = 0;            // highest snapshot sequence applied
    // recorded on the stream right before each batch's classify launch: once it completes, that launch is the next
    // thing the stream runs, and its snapshot follows within microseconds (blocking-sync: the host sleeps on it)
    hipEvent_t pre_launch = nullptr;
    bool use_event = true;
    uint32_t fin_cap = 0;  // finalize workgroups at most (0: one per CU; PPE_FLOW_FIN_WGS, default half the CUs)
    // ring over the last kSnapRing batches: packets submitted before batch b (of batches that may revoke: _rev)
    static constexpr uint32_t kSnapRing = 4096;
    std::vector<uint64_t> cum_n, cum_rev;
    uint64_t tot_n = 0, tot_rev = 0;
    // set when a batch's post-classify launch failed after its classify launch ran: that batch's claims were never
    // finalized (miss-tile counter, snapshot, creators), so every later call on the table fails until
    // ppe_flow_destroy / ppe_flow_create
    bool broken = false;
    // batches of at most PPE_FLOW_SMALL_CUTOFF packets take the one-launch kernel (PPE_FLOW_SMALL=0 at ppe_flow_create:
    // never, the A/B switch); what the last batch took, for ppe_flow_launch_info
    bool small_allowed = true;
    uint32_t last_kind = 0, last_launches = 0;
    // ppe_flow_stream_attach: StreamTcp's session machine behind the table (arr[].sess beside the slot arrays); the
    // batch's tuples when the caller asks for none (the session phase reads them)
    bool stream_on = false;
    uint32_t *tuple_scr = nullptr;
};

}  // namespace

// A launch that reads an image slot or a descriptor-ring slot, the last one per stream (streams run their launches in
// order): a classify launch is tracked by its sequence number, which its last workgroup publishes to pinned memory
// (ppe_kargs.done_*; no event marker behind the launch: a marker cost the F1 stream 4.5 µs per batch, r6o); other
// launches (ppe_acl_lookup) by an event recorded behind them.
struct Reader {
    hipStream_t s;
    hipEvent_t ev;  // nullptr: tracked by seq
    uint64_t seq;
};
constexpr uint32_t kDoneSlots = 4096;  // launch-completion slots (sequence numbers modulo this)

// ppe_portscan_create: the port-scan detector's table and batch scratch (csrc/ppe_portscan.hip)
struct ppe_portscan_table {
    ppe_ctx *ctx = nullptr;
    ppe_portscan_cfg_t cfg = {};
    uint64_t now_cycles = 0, now_seconds = 0;   // ppe_portscan_clock
    unsigned long long *keys = nullptr, *recs = nullptr, *ctl = nullptr;
    uint32_t nslots = 0, npad_max = 0, rebuilds = 0;
    uint64_t occ_ub = 0;          // upper bound of the keys in use (the last count read + packets enqueued since)
    uint32_t *slot_of = nullptr, *dport = nullptr, *cbase = nullptr, *work = nullptr;
    uint64_t *pts = nullptr;
    unsigned long long *skey = nullptr, *cmask = nullptr, *mask = nullptr;
    uint8_t *res = nullptr;
    size_t mask_cap = 0;          // words of `mask`: the drop masks of the batches of one launch
    int fused_ok = 1;             // PPE_PS_FUSED at creation: 0 = every batch takes the staged launches
    uint32_t last_kind = 0, last_launches = 0;  // ppe_portscan_prepass_info: the last batch's pre-pass
    char err[256] = {0};
};

// ppe_attack_create: the attack monitors' rules, clock and device state (csrc/ppe_attack.hip, ppe_internal.h PPE_ATK_*)
struct ppe_attack {
    ppe_ctx *ctx = nullptr;
    ppe_attack_cfg_t cfg = {};
    uint64_t now = 0;                       // ppe_attack_clock / _tick
    unsigned long long *d_st = nullptr;     // [PPE_ATK_WORDS]
    unsigned long long *d_slots = nullptr;  // [ctx->max_grid][PPE_ATK_SLOT_WORDS] the classify workgroups' count slots
    const uint8_t **d_ports = nullptr;      // ppe_attack_ports: the device table launches read, or NULL
    std::vector<const uint8_t *> h_ports;   // its host copy (the port-scan pre-pass takes a batch's pointer by value)
    struct Retired { void *p; hipEvent_t done; };
    std::vector<Retired> retired;           // earlier tables, which launches in flight may still read: each is freed once
                                            // the event recorded behind the last launch that could read it has completed
    hipStream_t stream = nullptr;           // the context's latest classify stream: set / tick / clear go there
    char err[256] = {0};
};

struct ppe_ctx {
    int device = 0;
    uint32_t n_cu = 256;
    // classifier images
    uint32_t *d_img[2] = {nullptr, nullptr};
    size_t img_cap[2] = {0, 0};
    std::vector<uint32_t> h_img[2];
    // per image: its launch plan under `tune`, stateless / flow-table (csrc/launch_plan.cpp), and that plan's resident
    // workgroups per CU (0: not asked yet, blocks_per_cu)
    ppe_plan plan[2][2] = {};
    uint32_t plan_bpc[2][2] = {};
    ppe_acl_stats_t stats[2];
    hipEvent_t img_done[2] = {nullptr, nullptr};
    std::vector<Reader> img_readers[2];  // per slot: launch streams, their last launch with it
    hipStream_t aux = nullptr;                 // image uploads
    int running = 0;
    int staged = -1;              // ppe_rules_stage: the slot holding an unpublished image (-1: none)
    uint32_t rule_slots[2] = {0, 0};  // per image: the rule array length it was built from (acl_hit < this)
    uint64_t stage_token = 0, tokens = 0;
    // counters
    unsigned long long *d_cslots = nullptr;
    unsigned long long *d_sslots = nullptr;  // StreamTcp counter slots, [kSlotSets][max_grid][PPE_SSLOT_WORDS]
    ppe_stream_tcp_cfg_t stcp = {0u, 0u, 0u, 0u};  // ppe_stream_tcp_set: off until set
    uint32_t max_grid = 0;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;  // pairs
    size_t ev_used = 0;
    // host pipeline
    HostStage hs[kHostStreams];
    // ppe_classify_host_ordered: the one stream every chunk's pre-pass and classify launch goes to, and per staging
    // slot the events behind its upload and its launch
    hipStream_t host_cs = nullptr;
    hipEvent_t host_ev[kHostStreams][2] = {};
    // PPE_HOST_ORDERED_COPY at context creation: 0 the copies on host_cs too, 1 on the slots' streams with an event each
    // way.  One stream is faster at every size measured (pageable, 64 packets 72 vs 95 us, 262,144 in chunks of 16,384
    // 2.97 vs 3.41 ms, tools/ab_portscan_small.py): the detector's launches leave no room to overlap a copy with
    int host_ordered_copy = 0;
    // device-batch pipeline (ppe_classify_batches): consecutive batches alternate over these streams
    hipStream_t pipe[kPipeStreams] = {};
    hipEvent_t pipe_ev[kPipeStreams + 1] = {};
    int pipe_mode = 1;  // PPE_PIPE_MODE at context creation (see ppe_classify_batches)
    // descriptor rings of launches over more than PPE_MAX_BATCH batches: two slots used alternately; a slot is
    // rewritten only after every launch that read it has completed (one event per slot and reading stream, like the
    // image slots); a launch on another stream that reuses a slot's content waits only for its upload (ring_up)
    ppe_bdesc *d_ring[2] = {nullptr, nullptr};
    ppe_bdesc *h_ring[2] = {nullptr, nullptr};  // pinned staging of the H2D descriptor copy
    std::vector<Reader> ring_readers[2];
    // launch completions (struct Reader): pinned words the launches' last workgroups write, device running counts
    volatile unsigned long long *done_h = nullptr;
    unsigned long long *done_hd = nullptr, *done_cnt = nullptr;
    uint64_t done_cum[kDoneSlots] = {};  // per slot: the running workgroup count its next launch completes
    uint64_t launch_seq = 0;
    hipEvent_t ring_up[2] = {nullptr, nullptr};  // behind the slot's last upload, on ring_up_stream
    hipStream_t ring_up_stream[2] = {nullptr, nullptr};
    uint32_t ring_n[2] = {0, 0};       // descriptors the slot holds (its content = h_ring[slot][0, ring_n))
    int ring_next = 0;
    std::vector<ppe_bdesc> ring_tmp;   // descriptors of the launch being built
    ppe_tuning_t tune;
    // batch groups of waves a launch may split into (PPE_GROUPS): more groups = more tiles per wave between batch
    // setups, but more batches streamed at once (DRAM locality); C1, 20-32 batches per launch, per batch: 1 / 2 / 4
    // / 8 / 32 groups 20.2 / 18.7 / 18.3 / 18.3 / 19.1 us (one run, tools/ab_bench.py)
    uint32_t max_groups = 8;
    ppe_portscan_table *ps = nullptr;  // ppe_portscan_attach
    ppe_portscan_table *ps_flow = nullptr;  // ppe_flow_portscan_attach: ppe_classify_flow's detector (never the same table as ps)
    ppe_attack *atk = nullptr;         // ppe_attack_attach
    ppe_attack *atk_flow = nullptr;    // ppe_flow_attack_attach: ppe_classify_flow's monitors (never the same object as atk)
    uint32_t flow_combine = 0;         // ppe_flow_combine: ps_flow (able 1) and atk_flow on one batch, in one launch
    uint32_t flow_st_monitors = 0;     // ppe_flow_stream_monitors: atk_flow and the sessions on one batch, in one launch
    uint32_t flow_st_portscan = 0;     // ppe_flow_stream_portscan: ps_flow (able 1) and the sessions on one batch, in one launch
    unsigned long long *d_stc = nullptr;  // the session path's counter block (PPE_STC_WORDS), from the first attach on
    FlowTable *flow = nullptr;  // ppe_flow_create
    LookupStage lk;             // ppe_acl_lookup_host
    uint32_t *d_steer = nullptr;  // ppe_steer_partition: per-tile owner counts / offsets
    size_t steer_cap = 0;
    char err[256] = {0};
};

namespace {

int fail(ppe_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof c->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(c, expr)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail((c), PPE_EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// Kernel variant knobs live per context (ppe_set_tuning); the defaults are the fastest measured on MI355X
//  and can be overridden by PPE_BLOCK / PPE_BLOCKS_PER_CU / PPE_LDS_IMG.
ppe_tuning_t default_tuning() {
    ppe_tuning_t t;
    const int b = env_int("PPE_BLOCK", 0);
    t.block = (uint32_t)(b == 256 || b == 512 || b == 1024 ? b : 0);  // 0 = chosen per image
    const int bpc = env_int("PPE_BLOCKS_PER_CU", 0);
    t.blocks_per_cu = bpc > 0 && bpc <= (int)kMaxBlocksPerCU ? (uint32_t)bpc : 0u;
    const int pl = env_int("PPE_PIPELINE", 0);
    t.pipeline = pl == 1 || pl == 3 || pl == 4 || pl == 5 ? (uint32_t)pl : 0u;
    t.lds_image = env_int("PPE_LDS_IMG", 1) != 0 ? 1u : 0u;
    t.batches_per_launch = (uint32_t)std::max(0, std::min(env_int("PPE_BATCHES_PER_LAUNCH", (int)kBatchesPerLaunch),
                                                          PPE_MAX_RING));
    return t;
}

// Resident workgroups per CU of slot r's plan (fl: its flow-table plan): the occupancy API's answer (register and LDS
// limits) unless the tuning fixes it.  The persistent grid is CUs × this, so no workgroup waits for a second round.
// The occupancy query costs microseconds of host time: asked on the plan's first launch and kept with the plan (a
// flow-table launch: the flow variant's own occupancy, so its grid is resident in one round and each workgroup's
// owner-update buckets hold as many entries as it can)
uint32_t blocks_per_cu(ppe_ctx *c, int r, bool fl = false) {
    const ppe_plan &p = c->plan[r][fl];
    const uint32_t cap = kMaxBlocksPerCU * 256u / p.block;
    if (c->tune.blocks_per_cu) return std::max(1u, std::min(c->tune.blocks_per_cu, cap));  // may exceed residency
    uint32_t &bpc = c->plan_bpc[r][fl];
    if (!bpc) {
        const int occ = fl ? ppe_classify_occupancy_flow(p.stage_words, (int)p.mode, (int)p.block)
                           : ppe_classify_occupancy(p.stage_words, (int)p.mode, (int)p.pipe, (int)p.block);
        bpc = occ > 0 ? std::min<uint32_t>((uint32_t)occ, cap) : 1u;
    }
    return bpc;
}

// The plans of slot r's image under the context's tuning (after an upload or a tuning change)
int plan_slot(ppe_ctx *c, int r) {
    for (int fl = 0; fl < 2; ++fl) {
        if (ppe_plan_image(c->h_img[r].data(), (uint32_t)c->h_img[r].size(), &c->tune, fl, &c->plan[r][fl]) != PPE_OK)
            return fail(c, PPE_EINVAL, "no launch plan for the classifier image in slot %d", r);
        c->plan_bpc[r][fl] = 0;
    }
    return PPE_OK;
}

// A launch on stream s reads slot r of an image or descriptor ring: an event (one per slot and stream) is recorded
// behind it, so a rewrite of the slot waits for exactly the launches that read it (the event outlives the stream if
// the caller frees it).  Events of other streams whose launches have completed are dropped once the list grows, so a
// caller that uses a new stream per call does not make the list (and every later rewrite's wait) grow without bound.
// ---- readers of image / descriptor-ring slots (struct Reader) --------------------------------------------------------
static bool launch_done(const ppe_ctx *c, uint64_t seq) { return c->done_h[seq % kDoneSlots] >= seq; }

// a tracked launch's completion: the pinned word its last workgroup writes, polled (the core yielded between polls,
// as for the flow snapshot), bounded; past the bound the device is synchronised and the word read once more
static int wait_launch(ppe_ctx *c, uint64_t seq) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(30);
    while (!launch_done(c, seq)) {
        if (std::chrono::steady_clock::now() > until) {
            HIPCHK(c, hipDeviceSynchronize());
            if (!launch_done(c, seq)) return fail(c, PPE_EIO, "launch %llu never reported its completion", (unsigned long long)seq);
            break;
        }
        sched_yield();
    }
    return PPE_OK;
}
static bool reader_done(const ppe_ctx *c, const Reader &x) {
    return x.ev ? hipEventQuery(x.ev) == hipSuccess : launch_done(c, x.seq);
}
static int wait_reader(ppe_ctx *c, Reader &x) {
    if (!x.ev) return wait_launch(c, x.seq);   // (an entry with an event: its event is behind any seq it had)
    HIPCHK(c, hipEventSynchronize(x.ev));
    return PPE_OK;
}
static void drop_readers(std::vector<Reader> &v) {
    for (auto &x : v)
        if (x.ev) (void)hipEventDestroy(x.ev);
    v.clear();
}
// stream s's entry (created empty), after pruning other streams' completed ones
static Reader &reader_of(const ppe_ctx *c, std::vector<Reader> &readers, hipStream_t s) {
    constexpr size_t kPruneAt = 8;
    if (readers.size() >= kPruneAt) {
        size_t k = 0;
        for (size_t i = 0; i < readers.size(); ++i) {
            Reader &x = readers[i];
            if (x.s != s && reader_done(c, x)) {
                if (x.ev) (void)hipEventDestroy(x.ev);
                continue;
            }
            readers[k++] = x;
        }
        readers.resize(k);
    }
    for (auto &x : readers)
        if (x.s == s) return x;
    readers.push_back(Reader{s, nullptr, 0});
    return readers.back();
}
// a tracked classify launch (sequence number seq) read the slot on stream s: it completes after every earlier launch
// on s, so it replaces their entry
static void note_launch_reader(ppe_ctx *c, std::vector<Reader> &readers, hipStream_t s, uint64_t seq) {
    Reader &x = reader_of(c, readers, s);
    if (x.ev) (void)hipEventDestroy(x.ev);
    x.ev = nullptr;
    x.seq = seq;
}
// an untracked launch read the slot on stream s: an event behind it
int note_reader(ppe_ctx *c, std::vector<Reader> &readers, hipStream_t s) {
    Reader &x = reader_of(c, readers, s);
    if (!x.ev) HIPCHK(c, hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(x.ev, s));
    return PPE_OK;
}
int note_image_reader(ppe_ctx *c, int r, hipStream_t s) { return note_reader(c, c->img_readers[r], s); }

// the next tracked launch's sequence number and completion slot, in its kernel arguments (the slot's previous launch,
// kDoneSlots launches ago, has completed: at most one launch per slot in flight)
static int track_launch(ppe_ctx *c, uint32_t grid, ppe_kargs &a) {
    const uint64_t seq = c->launch_seq + 1u;
    const uint32_t q = (uint32_t)(seq % kDoneSlots);
    if (seq > kDoneSlots) {
        const int rc = wait_launch(c, seq - kDoneSlots);
        if (rc != PPE_OK) return rc;
    }
    c->launch_seq = seq;
    c->done_cum[q] += grid;
    a.done_cnt = c->done_cnt + q;
    a.done_host = c->done_hd + q;
    a.done_target = c->done_cum[q];
    a.done_seq = seq;
    return PPE_OK;
}
// the launch did not start: its slot is completed by hand (its workgroups will never count)
static void untrack_launch(ppe_ctx *c, uint32_t grid, const ppe_kargs &a) {
    const uint32_t q = (uint32_t)(a.done_seq % kDoneSlots);
    c->done_cum[q] -= grid;
    c->done_h[q] = a.done_seq;
}

int upload_image(ppe_ctx *c, int slot, uint32_t *words, uint32_t n_words, const ppe_acl_stats_t *st) {
    // The back image may still be read by launches queued before the previous swap.  Wait for exactly those (the
    // events recorded behind them, note_image_reader): unrelated work on any stream is never waited on.
    for (auto &x : c->img_readers[slot]) {
        const int rc = wait_reader(c, x);
        if (rc != PPE_OK) return rc;
    }
    drop_readers(c->img_readers[slot]);
    if (!c->aux) HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    const size_t bytes = (size_t)n_words * 4u;
    if (bytes > c->img_cap[slot]) {
        // (grown with headroom: a growing rule set reallocates rarely; the free of an unused slot is then safe)
        const size_t cap = std::max(bytes + bytes / 2, (size_t)64 * 1024);
        if (c->d_img[slot]) HIPCHK(c, hipFree(c->d_img[slot]));
        c->d_img[slot] = nullptr;
        HIPCHK(c, hipMalloc(&c->d_img[slot], cap + 64));
        c->img_cap[slot] = cap;
    }
    // the copy runs on the engine's own non-blocking stream: no implicit synchronisation with other streams
    HIPCHK(c, hipMemcpyAsync(c->d_img[slot], words, bytes, hipMemcpyHostToDevice, c->aux));
    HIPCHK(c, hipStreamSynchronize(c->aux));
    c->h_img[slot].assign(words, words + n_words);
    c->stats[slot] = *st;
    const int rc = plan_slot(c, slot);
    c->stats[slot].lds_resident = c->plan[slot][0].mode;
    return rc;
}

// What the batches of one launch need of the grid and allow of the kernel variant
struct BatchShape {
    uint32_t tiles = 0;        // largest batch's tile count
    uint64_t tiles_total = 0;
    bool part = true;          // the throughput layout in every batch (ppe_kargs.part_layout)
};

// The descriptors d[0..nb) of batches in / out [0..nb) (fl: a flow-table launch), over image slot r
int fill_descs(ppe_ctx *c, int r, const ppe_batch_t *in, const ppe_result_t *out, uint32_t nb, uint32_t idx_base,
               bool fl, ppe_bdesc *descs, BatchShape &sh, bool psc = false) {
    uint32_t ps_off = 0;  // port-scan launches: the batches' drop masks lie one after the other (ps_prepass)
    for (uint32_t i = 0; i < nb; ++i) {
        ppe_bdesc &d = descs[i];
        d.hdr = in[i].hdr;
        d.len = in[i].len;
        d.ts = in[i].ts;
        d.n = in[i].n;
        d.stride = in[i].stride;
        d.verdict = out[i].verdict;
        d.fhash = out[i].flow_hash;
        d.hit = out[i].acl_hit;
        d.fw_idx = out[i].fw_idx;
        d.drop_idx = out[i].drop_idx;
        d.tile_cnt = out[i].tile_cnt;
        d.tuple = out[i].tuple;
        d.idx_base = idx_base;
        d.flags = 0;
        if (out[i].part8) {
            if (d.fw_idx || d.drop_idx || d.tile_cnt)
                return fail(c, PPE_EINVAL, "part8 replaces fw_idx / drop_idx / tile_cnt (pass them NULL)");
            d.tile_cnt = (uint32_t *)out[i].part8;  // (the kernel reads the compact list from the tile_cnt field)
            d.flags = PPE_BD_PART8;
        }
        if (out[i].packed) {
            if (d.verdict || d.fhash || d.hit)
                return fail(c, PPE_EINVAL, "packed replaces verdict / flow_hash / acl_hit (pass them NULL)");
            if (fl) return fail(c, PPE_EINVAL, "the packed result layout is for ppe_classify / ppe_classify_batches");
            if (c->rule_slots[r] > PPE_PACKED_MAX_RULES)
                return fail(c, PPE_EINVAL, "packed results hold rule indices below %u (classifier of %u rule slots)",
                            PPE_PACKED_MAX_RULES, c->rule_slots[r]);
            d.verdict = (uint32_t *)out[i].packed;  // (the kernel writes the 8-B words through the verdict field)
            d.flags |= PPE_BD_PACKED;
        }
        sh.part = sh.part && ((d.verdict && d.fhash && d.hit) || (d.flags & PPE_BD_PACKED)) && !d.tuple &&
                  ((d.fw_idx && d.fw_idx == d.drop_idx && !d.tile_cnt) || (d.flags & PPE_BD_PART8));
        if (psc) {
            d.flags |= ps_off << PPE_BD_PSOFF_SHIFT;
            ps_off += (in[i].n + 63u) / 64u;
        }
        sh.tiles = std::max(sh.tiles, (in[i].n + 63u) / 64u);
        sh.tiles_total += (uint64_t)((in[i].n + 63u) / 64u);
    }
    return PPE_OK;
}

// The descriptor-ring slot a launch on stream s reads c->ring_tmp[0, nb) from.  A slot already holding exactly these
// descriptors is reused as is (a dataplane cycling over a fixed set of batch buffers uploads its descriptor table
// once); otherwise the next slot is rewritten once the launch that last read it (two ring launches ago) has completed
int pick_ring_slot(ppe_ctx *c, uint32_t nb, hipStream_t s, int &rslot) {
    const std::vector<ppe_bdesc> &rd = c->ring_tmp;
    const size_t bytes = sizeof(ppe_bdesc) * nb;
    bool ring_copy = false;
    rslot = -1;
    for (int k = 0; k < 2; ++k)
        if (c->ring_n[k] == nb && c->h_ring[k] && std::memcmp(c->h_ring[k], rd.data(), bytes) == 0) rslot = k;
    if (rslot < 0) {
        rslot = c->ring_next;
        c->ring_next ^= 1;
        for (auto &x : c->ring_readers[rslot]) {  // its last readers
            const int rc = wait_reader(c, x);
            if (rc != PPE_OK) return rc;
        }
        drop_readers(c->ring_readers[rslot]);
        std::memcpy(c->h_ring[rslot], rd.data(), bytes);
        c->ring_n[rslot] = nb;
        HIPCHK(c, hipMemcpyAsync(c->d_ring[rslot], c->h_ring[rslot], bytes, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->ring_up[rslot], s));
        c->ring_up_stream[rslot] = s;
        ring_copy = true;
    }
    if (!ring_copy && c->ring_up_stream[rslot] != s && hipEventQuery(c->ring_up[rslot]) != hipSuccess)
        HIPCHK(c, hipStreamWaitEvent(s, c->ring_up[rslot], 0));  // reused on another stream: after the upload only
    return PPE_OK;
}

int ps_fail(ppe_portscan_table *t, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t->err, sizeof t->err, fmt, ap);
    va_end(ap);
    if (t->ctx) std::snprintf(t->ctx->err, sizeof t->ctx->err, "%s", t->err);
    return code;
}
#define PSCHK(t, expr)                                                                               \
    do {                                                                                             \
        hipError_t e_ = (hipError_t)(expr);                                                          \
        if (e_ != hipSuccess) return ps_fail((t), PPE_EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

void ps_table_args(const ppe_portscan_table &t, ppe_ps_kargs &a) {
    std::memset(&a, 0, sizeof a);
    a.keys = t.keys;
    a.recs = t.recs;
    a.ctl = t.ctl;
    a.smask = t.nslots - 1u;
    a.capacity = t.cfg.capacity;
    a.rate = t.cfg.cycles_per_second;
    a.n = 1;
    a.npad = PPE_PS_SORT_BLOCK;
}

// Move the records that stay into an empty table: aging (age != 0: PortScan_timeout at now_cycles) and the
// reclamation of slots whose source never got a record.  Synchronises.
int ps_rebuild(ppe_portscan_table *t, int age, uint64_t now_cycles) {
    const size_t kb = (size_t)t->nslots * 8u, rb = kb * PPE_PS_REC_WORDS;
    unsigned long long *nk = nullptr, *nr = nullptr;
    if (hipMalloc(&nk, kb) != hipSuccess || hipMalloc(&nr, rb) != hipSuccess) {
        (void)hipFree(nk);
        return ps_fail(t, PPE_ENOMEM, "port-scan table rebuild: out of device memory");
    }
    ppe_ps_kargs a;
    ps_table_args(*t, a);
    a.dkeys = nk;
    a.drecs = nr;
    a.dmask = a.smask;
    a.age = age ? 1u : 0u;
    a.now_cycles = now_cycles;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(nk, 0, kb);
    if (e == hipSuccess) e = hipMemset(nr, 0, rb);
    if (e == hipSuccess) e = (hipError_t)ppe_launch_portscan(PPE_PS_K_REBUILD, &a, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long live = 0;
    if (e == hipSuccess) e = hipMemcpy(&live, t->ctl + PPE_PSC_LIVE, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(t->ctl + PPE_PSC_OCC, &live, 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(nk);
        (void)hipFree(nr);
        return ps_fail(t, PPE_EIO, "port-scan table rebuild: %s", hipGetErrorString(e));
    }
    (void)hipFree(t->keys);
    (void)hipFree(t->recs);
    t->keys = nk;
    t->recs = nr;
    t->occ_ub = live;
    ++t->rebuilds;
    return PPE_OK;
}

// Room for the keys a batch of n packets may claim: keys in use never reach 3/4 of the slots: the bound first, then the
// count, then a rebuild without aging
int ps_reserve_keys(ppe_portscan_table *t, uint32_t n) {
    if (t->occ_ub + n > (uint64_t)t->nslots / 4u * 3u) {
        PSCHK(t, hipDeviceSynchronize());
        unsigned long long occ = 0;
        PSCHK(t, hipMemcpy(&occ, t->ctl + PPE_PSC_OCC, 8, hipMemcpyDeviceToHost));
        t->occ_ub = occ;
        if (t->occ_ub + n > (uint64_t)t->nslots / 4u * 3u) {
            const int rc = ps_rebuild(t, 0, 0);
            if (rc != PPE_OK) return rc;
        }
    }
    t->occ_ub += n;
    return PPE_OK;
}

// PortScan_Detect for batches in[0, nb) in order on stream s (csrc/ppe_portscan.hip), their drop masks one after the
// other in t->mask
int ps_prepass(ppe_ctx *c, const ppe_batch_t *in, uint32_t nb, const ppe_cfg_t *cfg, hipStream_t s,
               uint32_t atk_pbase) {
    ppe_portscan_table *t = c->ps;
    size_t words = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        if (in[i].n > t->cfg.max_batch)
            return fail(c, PPE_EINVAL, "batch of %u packets exceeds the port-scan table's max_batch %u", in[i].n,
                        t->cfg.max_batch);
        words += (in[i].n + 63u) / 64u;
    }
    if (words > t->mask_cap) {  // (grows only: the masks of a launch over many batches)
        PSCHK(t, hipDeviceSynchronize());
        (void)hipFree(t->mask);
        t->mask = nullptr;
        t->mask_cap = 0;
        PSCHK(t, hipMalloc(&t->mask, words * 8u));
        t->mask_cap = words;
    }
    size_t off = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t n = in[i].n;
        const int krc = ps_reserve_keys(t, n);
        if (krc != PPE_OK) return krc;
        ppe_ps_kargs a;
        ps_table_args(*t, a);
        a.hdr = in[i].hdr;
        a.len = in[i].len;
        a.ts = in[i].ts;
        a.n = n;
        a.stride = in[i].stride;
        a.syn_check = cfg ? cfg->syn_check : 1u;
        a.ts_default = cfg ? cfg->now_seconds : 0u;
        uint32_t npad = PPE_PS_SORT_BLOCK;
        while (npad < n) npad <<= 1;
        a.npad = npad;
        a.now_cycles = t->now_cycles;
        a.now_seconds = t->now_seconds;
        a.freq = t->cfg.exception_freq;
        a.hold_seconds = t->cfg.hold_seconds;
        a.action = t->cfg.action;
        a.slot_of = t->slot_of;
        a.dport = t->dport;
        a.pts = t->pts;
        a.skey = t->skey;
        a.res = t->res;
        a.cmask = t->cmask;
        a.cbase = t->cbase;
        a.work = t->work;
        a.mask = t->mask + off;
        if (c->atk) {  // a packet the attack monitors drop never reaches the detector
            a.atk_st = c->atk->d_st;
            const size_t k = (size_t)atk_pbase + i;
            a.atk_ports = k < c->atk->h_ports.size() ? c->atk->h_ports[k] : nullptr;
        }
        off += (n + 63u) / 64u;
        if (ppe_pick_portscan_prepass(n, t->fused_ok)) {  // a small batch: every phase in one launch of one workgroup
            PSCHK(t, ppe_launch_portscan(PPE_PS_K_FUSED, &a, s));
            t->last_kind = 1u;
            t->last_launches = 1u;
            continue;
        }
        uint32_t launches = 10u;  // pre, post
        static const int pre[] = {PPE_PS_K_FIND, PPE_PS_K_CREATORS, PPE_PS_K_SCAN, PPE_PS_K_GRANT, PPE_PS_K_KEYS,
                                  PPE_PS_K_SORT_LDS};
        for (int k : pre) PSCHK(t, ppe_launch_portscan(k, &a, s));
        for (uint32_t k = 2u * PPE_PS_SORT_BLOCK; k <= npad && k; k <<= 1) {
            a.sort_k = k;
            for (uint32_t j = k >> 1; j >= PPE_PS_SORT_BLOCK; j >>= 1) {
                a.sort_j = j;
                PSCHK(t, ppe_launch_portscan(PPE_PS_K_SORT_GLOBAL, &a, s));
                ++launches;
            }
            PSCHK(t, ppe_launch_portscan(PPE_PS_K_SORT_MERGE_LDS, &a, s));
            ++launches;
        }
        static const int post[] = {PPE_PS_K_HEADS, PPE_PS_K_MEMBERS, PPE_PS_K_WALK, PPE_PS_K_MASK};
        for (int k : post) PSCHK(t, ppe_launch_portscan(k, &a, s));
        t->last_kind = 0u;
        t->last_launches = launches;
    }
    return PPE_OK;
}

// One launch over batches in[0..nb) (nb <= PPE_MAX_RING, each n > 0): every wave takes its tiles of batch 0, then
// of batch 1, ... (no barrier between batches, one image staging for all of them).
// small (flow-table launches only): the one-launch kernel of one 1024-thread workgroup, classify then finalize, with
// finalize's own arguments; with fps, the one-launch kernel with the port-scan detector inside and its arguments
// (fps_atk: the one with the flow-attached monitors in it as well); small_atk: the one-launch kernel of small with
// the flow-attached monitors in it; fatk_pb_set: the flow-attached monitors read the port bytes fatk_pb (device
// pointer or NULL) instead of the sticky table's entry 0; fst (with small): the one-launch kernel with the TCP session
// machine behind it and its arguments (fst_atk: the one with the flow-attached monitors in it as well); fps and fst
// together: the detector kernel with the session phase behind it (fst_atk: with the monitors in it as well)
int launch(ppe_ctx *c, const ppe_batch_t *in, const ppe_result_t *out, uint32_t nb, const ppe_cfg_t *cfg,
           hipStream_t s, int slot_set, uint32_t idx_base = 0, const ppe_flowdev *fl = nullptr,
           uint32_t *grid_out = nullptr, uint32_t atk_pbase = 0, const ppe_flow_small_tail *small = nullptr,
           const ppe_ps_kargs *fps = nullptr, bool fps_atk = false, bool small_atk = false,
           const uint8_t *fatk_pb = nullptr, bool fatk_pb_set = false, const ppe_flow_st_args *fst = nullptr,
           bool fst_atk = false) {
    const int r = c->running;
    const ppe_plan &plan = c->plan[r][fl != nullptr];
    ppe_kargs a;
    std::memset(&a, 0, sizeof a);
    const bool use_ring = nb > PPE_MAX_BATCH;
    if (use_ring) {
        if (nb > PPE_MAX_RING) return fail(c, PPE_EINVAL, "more than %d batches in one launch", PPE_MAX_RING);
        c->ring_tmp.resize(nb);
    }
    BatchShape sh;
    const bool psc = ppe_pick_portscan(fl != nullptr, c->ps != nullptr, c->ps ? c->ps->cfg.able : 0u) != 0u;
    int rc = fill_descs(c, r, in, out, nb, idx_base, fl != nullptr, use_ring ? c->ring_tmp.data() : a.batch, sh, psc);
    if (rc != PPE_OK) return rc;
    if (psc) {  // PortScan_Detect for every batch, in order, ahead of the launch on its stream
        rc = ps_prepass(c, in, nb, cfg, s, atk_pbase);
        if (rc != PPE_OK) return rc;
        a.psmask = c->ps->mask;
    }
    if (ppe_pick_attack(fl != nullptr, c->atk != nullptr)) {  // the monitors: rules and state on the device, clock by value
        ppe_attack *t = c->atk;
        a.atk_st = t->d_st;
        a.atk_slots = t->d_slots;
        a.atk_ports = t->d_ports;
        a.atk_nports = (uint32_t)t->h_ports.size();
        a.atk_pbase = atk_pbase;
        a.atk_now = t->now;
        a.atk_hold = t->cfg.hold_seconds;
        t->stream = s;
    }
    if (ppe_pick_attack_flow(fl != nullptr, c->atk_flow != nullptr)) {  // the same for the flow-table launch (one batch)
        ppe_attack *t = c->atk_flow;
        a.fatk_st = t->d_st;
        a.fatk_slots = t->d_slots;
        a.fatk_pb = fatk_pb_set ? fatk_pb : t->h_ports.empty() ? nullptr : t->h_ports[0];
        a.fatk_now = t->now;
        a.fatk_hold = t->cfg.hold_seconds;
        t->stream = s;
    }
    int rslot = 0;
    if (use_ring) {
        rc = pick_ring_slot(c, nb, s, rslot);
        if (rc != PPE_OK) return rc;
        a.batch[0] = c->ring_tmp[0];
        a.ring = c->d_ring[rslot];
    }
    ppe_plan_apply(&a, &plan);
    a.nbatch = nb;
    a.max_tiles = sh.tiles;
    a.part_layout = (sh.part && !fl && !env_int("PPE_NO_PART", 0)) ? 1u : 0u;
    a.max_groups = ppe_pick_groups(nb, c->max_groups);
    a.img = c->d_img[r];
    a.unsup_fw = cfg ? cfg->unsupport_proto_action : 0u;
    a.syn_check = cfg ? cfg->syn_check : 1u;
    a.now = cfg ? cfg->now_seconds : 0u;
    a.cslots = c->d_cslots + (size_t)slot_set * c->max_grid * PPE_CSLOT_WORDS;
    a.sslots = c->d_sslots + (size_t)slot_set * c->max_grid * PPE_SSLOT_WORDS;
    a.stream = (c->stcp.track && !fl)
                   ? PPE_STM_TRACK | ((c->stcp.midstream | c->stcp.async_oneside) ? PPE_STM_PICKUP : 0u) : 0u;
    if (fl) a.flow = *fl;
    // enough workgroups for every tile of every batch (the kernel splits its waves into batch groups), at most
    // the resident grid
    const uint32_t wpb = plan.block / 64u;
    const uint32_t want = (uint32_t)std::min<uint64_t>((sh.tiles_total + wpb - 1) / wpb, 1u << 30);
    const uint32_t maxg = c->n_cu * blocks_per_cu(c, r, fl != nullptr);
    const uint32_t grid = small ? 1u : std::max(1u, std::min(want, std::min(maxg, c->max_grid)));
    if (grid_out) *grid_out = grid;

    // the timing events are taken before the launch takes its completion slot: nothing between track_launch and the
    // launch call can return (a slot taken by a launch that never started would count as in flight for ever)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing) {
        if (c->ev_used + 2 > c->ev.size()) {
            for (int i = 0; i < 256; ++i) {
                hipEvent_t e;
                HIPCHK(c, hipEventCreate(&e));
                c->ev.push_back(e);
            }
        }
        e0 = c->ev[c->ev_used];
        e1 = c->ev[c->ev_used + 1];
    }
    rc = track_launch(c, grid, a);
    if (rc != PPE_OK) return rc;
    rc = (fps && fst && fst_atk)
             ? ppe_launch_flow_stream_portscan_attack(&a, small, fps, fst, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : (fps && fst) ? ppe_launch_flow_stream_portscan(&a, small, fps, fst, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : fst_atk ? ppe_launch_flow_stream_attack(&a, small, fst, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : fst   ? ppe_launch_flow_stream(&a, small, fst, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : fps_atk ? ppe_launch_flow_portscan_attack(&a, small, fps, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : fps   ? ppe_launch_flow_portscan(&a, small, fps, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : small_atk ? ppe_launch_flow_small_attack(&a, small, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
         : small ? ppe_launch_flow_small(&a, small, (int)plan.mode, (void *)s, (void *)e0, (void *)e1)
                 : ppe_launch_classify(&a, grid, (int)plan.mode, (int)plan.pipe, (int)plan.block, fl != nullptr,
                                       (void *)s, (void *)e0, (void *)e1);
    if (rc != 0) {
        untrack_launch(c, grid, a);
        return fail(c, PPE_EIO, "kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (c->timing) c->ev_used += 2;  // (only a launch that started: ppe_timing_read reads both events)
    // the launch reads its image slot (and ring slot): a later rewrite waits for its completion
    if (use_ring) note_launch_reader(c, c->ring_readers[rslot], s, a.done_seq);
    note_launch_reader(c, c->img_readers[r], s, a.done_seq);
    return PPE_OK;
}

hipError_t use_device(ppe_ctx *c) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == c->device) return hipSuccess;
    return hipSetDevice(c->device);
}

int check_batch(ppe_ctx *c, const ppe_batch_t *in, const ppe_cfg_t *cfg) {
    if (!in) return fail(c, PPE_EINVAL, "null batch");
    // an ACK-only first packet with midstream pickup enters segment reassembly (stream-tcp.c:371-432): not built, and
    // only syn_check keeps such packets from StreamTcp
    if (c->stcp.track && c->stcp.midstream && cfg && cfg->syn_check == 0)
        return fail(c, PPE_ENOTSUP, "stream tracking with midstream pickup needs syn_check (ACK-only pickup is not built)");
    if (in->n == 0) return PPE_OK;
    if (!in->hdr || !in->len) return fail(c, PPE_EINVAL, "hdr/len required");
    if (in->stride < 64 || in->stride > 256 || in->stride % 16u)
        return fail(c, PPE_EINVAL, "stride must be a multiple of 16 from 64 to 256");
    // byte offsets inside the kernel are 32-bit, and partition-list entries keep the action in bits 31:30
    if ((uint64_t)in->n * in->stride >= (1ull << 31)) return fail(c, PPE_EINVAL, "batch too large (n * stride >= 2^31)");
    if (((uintptr_t)in->hdr & 15u) != 0) return fail(c, PPE_EINVAL, "hdr must be 16-byte aligned");
    if (cfg && cfg->unsupport_proto_action > 1) return fail(c, PPE_EINVAL, "unsupport_proto_action must be 0/1");
    if (cfg && cfg->syn_check > 1) return fail(c, PPE_EINVAL, "syn_check must be 0/1");
    return PPE_OK;
}

}  // namespace

extern "C" {

static int flow_stream_zero(ppe_ctx *c);  // (with the flow table, below)

int ppe_abi_version(void) { return PPE_ABI_VERSION; }

const char *ppe_last_error(ppe_ctx_t *ctx) { return ctx ? ctx->err : "null context"; }

int ppe_ctx_create(int device, ppe_ctx_t **out) {
    if (!out) return PPE_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PPE_ENODEV;
    if (device < 0 || device >= ndev) return PPE_ENODEV;
    ppe_ctx *c = new (std::nothrow) ppe_ctx();
    if (!c) return PPE_ENOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return PPE_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->n_cu = (uint32_t)prop.multiProcessorCount;
    c->max_grid = c->n_cu * kMaxBlocksPerCU;
    c->tune = default_tuning();
    c->max_groups = (uint32_t)std::max(1, env_int("PPE_GROUPS", 8));
    c->pipe_mode = env_int("PPE_PIPE_MODE", 1);
    c->host_ordered_copy = env_int("PPE_HOST_ORDERED_COPY", 0) != 0;
    const size_t cs_bytes = (size_t)kSlotSets * c->max_grid * PPE_CSLOT_WORDS * sizeof(unsigned long long);
    int rc = PPE_OK;
    if (hipMalloc(&c->d_cslots, cs_bytes) != hipSuccess || hipMemset(c->d_cslots, 0, cs_bytes) != hipSuccess)
        rc = PPE_ENOMEM;
    const size_t ss_bytes = (size_t)kSlotSets * c->max_grid * PPE_SSLOT_WORDS * sizeof(unsigned long long);
    if (rc == PPE_OK &&
        (hipMalloc(&c->d_sslots, ss_bytes) != hipSuccess || hipMemset(c->d_sslots, 0, ss_bytes) != hipSuccess))
        rc = PPE_ENOMEM;
    for (int i = 0; i < 2 && rc == PPE_OK; ++i)
        if (hipEventCreateWithFlags(&c->img_done[i], hipEventDisableTiming) != hipSuccess) rc = PPE_EIO;
    // launch completions (struct Reader): pinned, device-mapped words and the device running counts
    if (rc == PPE_OK) {
        void *h = nullptr;
        if (hipHostMalloc(&h, kDoneSlots * 8u, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void **)&c->done_hd, h, 0) != hipSuccess ||
            hipMalloc(&c->done_cnt, kDoneSlots * 8u) != hipSuccess || hipMemset(c->done_cnt, 0, kDoneSlots * 8u) != hipSuccess)
            rc = PPE_ENOMEM;
        c->done_h = (volatile unsigned long long *)h;
        if (h) std::memset(h, 0, kDoneSlots * 8u);
    }
    // descriptor ring slots (launches over more than PPE_MAX_BATCH batches): allocated here, not on first use, so
    // no batch call pays an allocation
    for (int i = 0; i < 2 && rc == PPE_OK; ++i)
        if (hipMalloc(&c->d_ring[i], sizeof(ppe_bdesc) * PPE_MAX_RING) != hipSuccess ||
            hipHostMalloc(&c->h_ring[i], sizeof(ppe_bdesc) * PPE_MAX_RING, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&c->ring_up[i], hipEventDisableTiming) != hipSuccess)
            rc = PPE_ENOMEM;
    if (rc == PPE_OK) {
        // empty rule set, management default action DROP (mgrplane/src/srv/srvnet/srv_rule.c:84)
        rc = ppe_rules_commit(c, nullptr, nullptr, 0, ACL_RULE_ACTION_DROP, nullptr);
    }
    if (rc != PPE_OK) {
        ppe_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return PPE_OK;
}

int ppe_ctx_destroy(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 2; ++i) {
        if (c->d_img[i]) (void)hipFree(c->d_img[i]);
        if (c->img_done[i]) (void)hipEventDestroy(c->img_done[i]);
    }
    if (c->d_cslots) (void)hipFree(c->d_cslots);
    if (c->d_sslots) (void)hipFree(c->d_sslots);
    if (c->d_stc) (void)hipFree(c->d_stc);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (c->d_ring[i]) (void)hipFree(c->d_ring[i]);
        if (c->h_ring[i]) (void)hipHostFree(c->h_ring[i]);
        if (c->ring_up[i]) (void)hipEventDestroy(c->ring_up[i]);
        drop_readers(c->ring_readers[i]);
    }
    for (hipStream_t s : c->pipe)
        if (s) (void)hipStreamDestroy(s);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    for (auto &v : c->img_readers) drop_readers(v);
    if (c->done_h) (void)hipHostFree((void *)c->done_h);
    if (c->done_cnt) (void)hipFree(c->done_cnt);
    for (hipEvent_t e : c->pipe_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->flow) ppe_flow_destroy(c);
    if (c->lk.s) (void)hipStreamDestroy(c->lk.s);
    if (c->lk.h) (void)hipHostFree(c->lk.h);
    if (c->d_steer) (void)hipFree(c->d_steer);
    if (c->host_cs) (void)hipStreamDestroy(c->host_cs);
    for (auto &pair : c->host_ev)
        for (hipEvent_t e : pair)
            if (e) (void)hipEventDestroy(e);
    for (auto &h : c->hs) {
        if (h.s) (void)hipStreamDestroy(h.s);
        (void)hipFree(h.hdr);
        (void)hipFree(h.len);
        (void)hipFree(h.ts);
        (void)hipFree(h.verdict);
        (void)hipFree(h.fhash);
        (void)hipFree(h.hit);
        (void)hipFree(h.fw);
        (void)hipFree(h.drop);
        (void)hipFree(h.tcnt);
        (void)hipFree(h.tuple);
        (void)hipFree(h.ports);
    }
    delete c;
    return PPE_OK;
}

int ppe_ctx_device(ppe_ctx_t *c) { return c ? c->device : PPE_EINVAL; }

int ppe_rules_stage(ppe_ctx_t *c, const RCP_BLOCK_ACL_RULE_TUPLE *rules, const uint8_t *used, uint32_t n,
                    uint32_t default_action, ppe_acl_stats_t *stats, uint64_t *token) {
    if (!c) return PPE_EINVAL;
    if (default_action > 0xffffu) return fail(c, PPE_EINVAL, "default action out of range");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t *words = nullptr, n_words = 0;
    ppe_acl_stats_t st;
    const char *bt = getenv("PPE_BINTH");
    const uint32_t binth = bt ? (uint32_t)atoi(bt) : 0u;
    int rc = ppe_acl_build_image(rules, used, n, default_action, binth, &words, &n_words, &st);
    if (rc != PPE_OK) return fail(c, rc, "classifier build failed (%d)", rc);
    // the back slot (the context's creation commits an image, so the running slot is never empty after it)
    const int back = c->h_img[c->running].empty() ? c->running : 1 - c->running;
    c->staged = -1;  // (an unpublished image there is replaced: its token no longer publishes)
    rc = upload_image(c, back, words, n_words, &st);
    ppe_acl_free_image(words);
    if (rc != PPE_OK) return rc;
    c->staged = back;
    c->rule_slots[back] = n;
    c->stage_token = ++c->tokens;
    if (token) *token = c->stage_token;
    if (stats) *stats = c->stats[back];
    return PPE_OK;
}

int ppe_rules_publish(ppe_ctx_t *c, uint64_t token) {
    if (!c) return PPE_EINVAL;
    if (token == 0 || c->staged < 0 || token != c->stage_token)
        return fail(c, PPE_EINVAL, "no staged classifier with token %llu", (unsigned long long)token);
    c->running = c->staged;  // later launches read the new image (set_running_acltree, dp_cmd.c:1980-1985)
    c->staged = -1;
    return PPE_OK;
}

int ppe_rules_commit(ppe_ctx_t *c, const RCP_BLOCK_ACL_RULE_TUPLE *rules, const uint8_t *used, uint32_t n,
                     uint32_t default_action, ppe_acl_stats_t *stats) {
    uint64_t token = 0;
    const int rc = ppe_rules_stage(c, rules, used, n, default_action, stats, &token);
    return rc != PPE_OK ? rc : ppe_rules_publish(c, token);
}

int ppe_classify(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                 void *stream) {
    if (!c || !out) return PPE_EINVAL;
    int rc = check_batch(c, in, cfg);
    if (rc != PPE_OK || in->n == 0) return rc;
    HIPCHK(c, use_device(c));
    return launch(c, in, out, 1, cfg, (hipStream_t)stream, 0);
}

int ppe_classify_batches(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, uint32_t nbatch,
                         const ppe_cfg_t *cfg, void *stream) {
    if (!c || (nbatch && (!in || !out))) return PPE_EINVAL;
    for (uint32_t i = 0; i < nbatch; ++i) {
        const int rc = check_batch(c, &in[i], cfg);
        if (rc != PPE_OK) return rc;
    }
    if (nbatch == 0) return PPE_OK;
    HIPCHK(c, use_device(c));
    const hipStream_t s = (hipStream_t)stream;
    const int mode = c->pipe_mode;
    const uint32_t per = c->tune.batches_per_launch ? std::min<uint32_t>(c->tune.batches_per_launch, PPE_MAX_RING)
                                                    : (uint32_t)PPE_MAX_RING;
    uint32_t nonempty = 0;
    for (uint32_t i = 0; i < nbatch; ++i) nonempty += in[i].n != 0;
    if (nonempty == 0) return PPE_OK;
    if (c->atk) {
        // attack monitors: the launches go one after the other on the caller's stream; a launch takes consecutive
        // batches of the call (an empty one ends it), so batch k keeps its port array ppe_attack_ports gave it
        std::vector<ppe_batch_t> gin;
        std::vector<ppe_result_t> gout;
        uint32_t base = 0;
        for (uint32_t i = 0; i <= nbatch; ++i) {
            if (i < nbatch && in[i].n) {
                if (gin.empty()) base = i;
                gin.push_back(in[i]);
                gout.push_back(out[i]);
            }
            if (!gin.empty() && (i == nbatch || in[i].n == 0 || gin.size() == per)) {
                const int rc = launch(c, gin.data(), gout.data(), (uint32_t)gin.size(), cfg, s, 0, 0, nullptr, nullptr,
                                      base);
                if (rc != PPE_OK) return rc;
                gin.clear();
                gout.clear();
            }
        }
        return PPE_OK;
    }
    if (nonempty <= per) {  // one launch: straight onto the caller's stream, no fork / join
        std::vector<ppe_batch_t> gin;
        std::vector<ppe_result_t> gout;
        gin.reserve(nonempty);
        gout.reserve(nonempty);
        for (uint32_t i = 0; i < nbatch; ++i)
            if (in[i].n) {
                gin.push_back(in[i]);
                gout.push_back(out[i]);
            }
        return launch(c, gin.data(), gout.data(), nonempty, cfg, s, 0);
    }
    if (c->ps && c->ps->cfg.able == 1u) {
        // the detector takes the batches in call order: the launches go one after the other on the caller's stream
        std::vector<ppe_batch_t> gin;
        std::vector<ppe_result_t> gout;
        for (uint32_t i = 0; i <= nbatch; ++i) {
            if (i < nbatch && in[i].n) {
                gin.push_back(in[i]);
                gout.push_back(out[i]);
            }
            if (gin.size() == per || (i == nbatch && !gin.empty())) {
                const int rc = launch(c, gin.data(), gout.data(), (uint32_t)gin.size(), cfg, s, 0);
                if (rc != PPE_OK) return rc;
                gin.clear();
                gout.clear();
            }
        }
        return PPE_OK;
    }
    if (!c->pipe[0]) {
        for (int k = 0; k < kPipeStreams; ++k)
            HIPCHK(c, hipStreamCreateWithFlags(&c->pipe[k], mode == 2 ? hipStreamDefault : hipStreamNonBlocking));
        for (hipEvent_t &e : c->pipe_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // mode 1: the caller's stream carries the even batches and one engine stream the odd ones; else two engine
    // streams.  fork: the engine streams start after the work already queued on `stream`
    hipStream_t q[kPipeStreams];
    for (int k = 0; k < kPipeStreams; ++k) q[k] = (mode == 1 && k == 0) ? s : c->pipe[k];
    HIPCHK(c, hipEventRecord(c->pipe_ev[kPipeStreams], s));
    for (int k = 0; k < kPipeStreams; ++k)
        if (q[k] != s) HIPCHK(c, hipStreamWaitEvent(q[k], c->pipe_ev[kPipeStreams], 0));
    // groups of up to PPE_MAX_BATCH non-empty batches per launch, launches alternating over the streams
    std::vector<ppe_batch_t> gin(std::min<uint32_t>(nbatch, PPE_MAX_RING));
    std::vector<ppe_result_t> gout(gin.size());
    uint32_t ng = 0, nl = 0;
    for (uint32_t i = 0; i <= nbatch; ++i) {
        if (i < nbatch && in[i].n == 0) continue;
        if (i < nbatch) {
            gin[ng] = in[i];
            gout[ng] = out[i];
            ++ng;
        }
        if (ng == per || (i == nbatch && ng)) {
            const int rc = launch(c, gin.data(), gout.data(), ng, cfg, q[nl % kPipeStreams], 0);
            if (rc != PPE_OK) return rc;
            ng = 0;
            ++nl;
        }
    }
    // join: `stream` continues after every batch
    for (int k = 0; k < kPipeStreams; ++k) {
        if (q[k] == s) continue;
        HIPCHK(c, hipEventRecord(c->pipe_ev[k], q[k]));
        HIPCHK(c, hipStreamWaitEvent(s, c->pipe_ev[k], 0));
    }
    return PPE_OK;
}

// device address of a pinned, device-mapped host buffer (hipHostMalloc / registered / torch pin_memory), or nullptr
static const void *mapped_host(const void *p) {
    if (!p) return nullptr;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error for the caller
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    return (const char *)at.devicePointer + ((const char *)p - (const char *)at.hostPointer);
}

// the staging slots of the host-buffer calls: a stream each, and device buffers for `chunk` packets of `stride` bytes
static int host_stages_reserve(ppe_ctx_t *c, uint32_t chunk, uint32_t stride) {
    for (auto &h : c->hs) {
        if (!h.s) HIPCHK(c, hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking));
        if (h.cap < chunk || h.stride != stride) {
            (void)hipFree(h.hdr); (void)hipFree(h.len); (void)hipFree(h.ts); (void)hipFree(h.verdict); (void)hipFree(h.fhash);
            (void)hipFree(h.hit); (void)hipFree(h.fw); (void)hipFree(h.drop); (void)hipFree(h.tcnt); (void)hipFree(h.tuple);
            (void)hipFree(h.ports);
            h = HostStage{h.s};
            HIPCHK(c, hipMalloc(&h.hdr, (size_t)chunk * stride));
            HIPCHK(c, hipMalloc(&h.len, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.ts, (size_t)chunk * 8));
            HIPCHK(c, hipMalloc(&h.verdict, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.fhash, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.hit, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.fw, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.drop, (size_t)chunk * 4));
            HIPCHK(c, hipMalloc(&h.tcnt, (size_t)(chunk / 64) * 4));
            HIPCHK(c, hipMalloc(&h.tuple, (size_t)chunk * 16));
            HIPCHK(c, hipMalloc(&h.ports, (size_t)chunk));
            h.cap = chunk;
            h.stride = stride;
        }
    }
    return PPE_OK;
}

// ppe_classify_host (ordered false: the chunks' launches on the staging slots' streams) and
// ppe_classify_host_ordered with the detector on (ordered: every chunk's pre-pass and classify launch on c->host_cs, in
// chunk order; the copies go to host_cs too, or stay on the slots' streams with an event each way)
static int classify_host_run(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                             uint32_t chunk, bool ordered) {
    int rc = check_batch(c, in, cfg);
    if (rc != PPE_OK || in->n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // Zero-copy: when every buffer is pinned and device-mapped, the kernel reads the windows and writes the results
    // across PCIe itself (C1: 822 vs 628 Mpps for the staged copies below, tools/host_zero_copy.py)
    const uint32_t ps_max = ordered ? c->ps->cfg.max_batch : 0u;  // the detector takes max_batch packets per launch
    if (ordered && ps_max < 64u)
        return fail(c, PPE_EINVAL, "ppe_classify_host_ordered: the port-scan table's max_batch is below one tile");
    if (env_int("PPE_HOST_ZEROCOPY", 1) && (!ordered || in->n <= ps_max)) {
        ppe_batch_t b = *in;
        ppe_result_t r = *out;
        bool ok = (b.hdr = (const uint8_t *)mapped_host(in->hdr)) && (b.len = (const uint32_t *)mapped_host(in->len));
        if (in->ts) ok = ok && (b.ts = (const uint64_t *)mapped_host(in->ts));
        uint32_t **outs[] = {&r.verdict, &r.flow_hash, (uint32_t **)&r.acl_hit, &r.fw_idx, &r.drop_idx, &r.tile_cnt,
                             &r.tuple, (uint32_t **)&r.part8, (uint32_t **)&r.packed};
        for (uint32_t **o : outs)
            if (ok && *o) ok = (*o = (uint32_t *)mapped_host(*o)) != nullptr;
        if (ok) {
            rc = launch(c, &b, &r, 1, cfg, nullptr, 0);
            if (rc != PPE_OK) return rc;
            HIPCHK(c, hipStreamSynchronize(nullptr));
            return PPE_OK;
        }
    }
    if (out->packed && out->tuple)  // (the staged path keeps the packed words in the tuple's staging buffer)
        return fail(c, PPE_EINVAL, "ppe_classify_host: packed with tuple needs device-mapped host buffers");
    if (chunk == 0) chunk = 1u << 18;
    chunk = (chunk + 63u) & ~63u;
    chunk = std::min(chunk, (in->n + 63u) & ~63u);
    if (ordered) {
        chunk = std::min(chunk, ps_max & ~63u);
        if (!c->host_cs) HIPCHK(c, hipStreamCreateWithFlags(&c->host_cs, hipStreamNonBlocking));
        if (c->host_ordered_copy)
            for (auto &pair : c->host_ev)
                for (hipEvent_t &e : pair)
                    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    rc = host_stages_reserve(c, chunk, in->stride);
    if (rc != PPE_OK) return rc;
    const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
    for (uint32_t base = 0, i = 0; base < in->n; base += chunk, ++i) {
        HostStage &h = c->hs[i % kHostStreams];
        hipEvent_t *ev = c->host_ev[i % kHostStreams];
        const hipStream_t ls = ordered ? c->host_cs : h.s;                           // the launches
        const hipStream_t xs = (ordered && !c->host_ordered_copy) ? c->host_cs : h.s;  // the copies
        const uint32_t m = std::min(chunk, in->n - base);
        HIPCHK(c, hipMemcpyAsync(h.hdr, in->hdr + (size_t)base * in->stride, (size_t)m * in->stride, h2d, xs));
        HIPCHK(c, hipMemcpyAsync(h.len, in->len + base, (size_t)m * 4, h2d, xs));
        if (in->ts) HIPCHK(c, hipMemcpyAsync(h.ts, in->ts + base, (size_t)m * 8, h2d, xs));
        ppe_batch_t b = {h.hdr, h.len, in->ts ? h.ts : nullptr, m, in->stride};
        ppe_result_t r;
        r.verdict = out->verdict ? h.verdict : nullptr;
        r.flow_hash = out->flow_hash ? h.fhash : nullptr;
        r.acl_hit = out->acl_hit ? h.hit : nullptr;
        const bool part = out->fw_idx && out->fw_idx == out->drop_idx;  // partition layout: one list
        r.fw_idx = out->fw_idx ? h.fw : nullptr;
        r.drop_idx = part ? h.fw : (out->drop_idx ? h.drop : nullptr);
        r.tile_cnt = out->tile_cnt ? h.tcnt : nullptr;
        r.tuple = out->tuple ? h.tuple : nullptr;
        r.part8 = out->part8 ? (uint8_t *)h.fw : nullptr;  // (part8 excludes fw_idx: the staging list is free)
        r.packed = out->packed ? (uint64_t *)h.tuple : nullptr;
        if (xs != ls) {  // the launch after the slot's upload, its download after the launch
            HIPCHK(c, hipEventRecord(ev[0], xs));
            HIPCHK(c, hipStreamWaitEvent(ls, ev[0], 0));
        }
        // (launches that follow each other on one stream share one counter slot set)
        rc = launch(c, &b, &r, 1, cfg, ls, ordered ? 1 : 1 + (int)(i % kHostStreams), base);
        if (rc != PPE_OK) return rc;
        if (xs != ls) {
            HIPCHK(c, hipEventRecord(ev[1], ls));
            HIPCHK(c, hipStreamWaitEvent(xs, ev[1], 0));
        }
        if (out->verdict) HIPCHK(c, hipMemcpyAsync(out->verdict + base, h.verdict, (size_t)m * 4, d2h, xs));
        if (out->flow_hash) HIPCHK(c, hipMemcpyAsync(out->flow_hash + base, h.fhash, (size_t)m * 4, d2h, xs));
        if (out->acl_hit) HIPCHK(c, hipMemcpyAsync(out->acl_hit + base, h.hit, (size_t)m * 4, d2h, xs));
        if (out->tuple) HIPCHK(c, hipMemcpyAsync(out->tuple + (size_t)base * 4, h.tuple, (size_t)m * 16, d2h, xs));
        if (out->tile_cnt)
            HIPCHK(c, hipMemcpyAsync(out->tile_cnt + base / 64, h.tcnt, (size_t)((m + 63) / 64) * 4, d2h, xs));
        // compacted indices carry the batch index (idx_base); chunk is a multiple of 64, so tiles line up
        if (out->fw_idx) HIPCHK(c, hipMemcpyAsync(out->fw_idx + base, h.fw, (size_t)m * 4, d2h, xs));
        if (out->drop_idx && !part)
            HIPCHK(c, hipMemcpyAsync(out->drop_idx + base, h.drop, (size_t)m * 4, d2h, xs));
        if (out->part8) HIPCHK(c, hipMemcpyAsync(out->part8 + base, h.fw, (size_t)m, d2h, xs));
        if (out->packed) HIPCHK(c, hipMemcpyAsync(out->packed + base, h.tuple, (size_t)m * 8, d2h, xs));
    }
    if (ordered) HIPCHK(c, hipStreamSynchronize(c->host_cs));
    for (auto &h : c->hs) HIPCHK(c, hipStreamSynchronize(h.s));
    return PPE_OK;
}

int ppe_classify_host(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                      uint32_t chunk) {
    if (!c || !out) return PPE_EINVAL;
    // the chunks of the staged path run on several streams; the detector needs the packets in order on one
    if (c->ps) return fail(c, PPE_ENOTSUP, "ppe_classify_host with a port-scan table attached is not supported");
    // the same for the attack monitors: their hold and their clock follow the order of the launches on one stream
    if (c->atk) return fail(c, PPE_ENOTSUP, "ppe_classify_host with attack monitors attached is not supported");
    return classify_host_run(c, in, out, cfg, chunk, false);
}

int ppe_classify_host_ordered(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                              uint32_t chunk) {
    if (!c || !out) return PPE_EINVAL;
    // the monitors' per-batch port arrays do not map onto chunks
    if (c->atk) return fail(c, PPE_ENOTSUP, "ppe_classify_host_ordered with attack monitors attached is not supported");
    // without the detector (no table, or portscan_able 0) the chunks are independent: ppe_classify_host's pipeline
    const bool psc = ppe_pick_portscan(0, c->ps != nullptr, c->ps ? c->ps->cfg.able : 0u) != 0u;
    return classify_host_run(c, in, out, cfg, chunk, psc);
}

int ppe_acl_lookup(ppe_ctx_t *c, const ppe_tuples_t *in, int32_t *hit, uint32_t *action, uint64_t now_seconds,
                   void *stream) {
    if (!c || !in) return PPE_EINVAL;
    if (in->n == 0) return PPE_OK;
    if (!in->tuple) return fail(c, PPE_EINVAL, "tuple required");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = c->running;
    const uint32_t words = c->h_img[r][PPE_IMG_W_OFFBSEC];  // the binary walk's part of the image (no blocks)
    // staging the image into each workgroup's LDS pays off over many tuples; a few (one flow miss's lookup) walk it
    // from L2 / HBM in one workgroup
    const bool lds = (size_t)words * 4u + 1024u <= PPE_LDS_IMG_MAX && in->n >= 4096u;
    ppe_tuple_kargs a;
    std::memset(&a, 0, sizeof a);
    a.tuple = in->tuple;
    a.macs = in->macs;
    a.ts = in->ts;
    a.n = in->n;
    a.hit = hit;
    a.action = action;
    a.img = c->d_img[r];
    a.img_words = words;
    a.default_action = c->h_img[r][PPE_IMG_W_DEFACT];
    a.now = now_seconds;
    const uint32_t want = (in->n + PPE_BLOCK - 1) / PPE_BLOCK;
    const uint32_t grid = std::max(1u, std::min(want, c->n_cu * 8u));
    const int rc = ppe_launch_acl_tuples(&a, grid, lds ? 1 : 0, stream);
    if (rc != 0) return fail(c, PPE_EIO, "acl kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return note_image_reader(c, r, (hipStream_t)stream);
}

int ppe_acl_lookup_host(ppe_ctx_t *c, const ppe_tuples_t *in, int32_t *hit, uint32_t *action,
                        uint64_t now_seconds) {
    if (!c || !in) return PPE_EINVAL;
    if (in->n == 0) return PPE_OK;
    if (!in->tuple) return fail(c, PPE_EINVAL, "tuple required");
    HIPCHK(c, use_device(c));
    LookupStage &L = c->lk;
    // the staging holds at most kLookupChunk entries (192 KB pinned per context, allocated by the first call); a
    // larger burst goes through it in chunks of that size
    constexpr uint32_t kLookupChunk = 4096;
    if (!L.s) HIPCHK(c, hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking));
    if (!L.h) {
        HIPCHK(c, hipHostMalloc((void **)&L.h, (size_t)kLookupChunk * 48u, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void **)&L.d, L.h, 0));
        L.cap = kLookupChunk;
    }
    const size_t cap = L.cap;
    uint8_t *ht = L.h, *hm = L.h + cap * 16, *hts = L.h + cap * 32, *hh = L.h + cap * 40, *ha = L.h + cap * 44;
    for (uint32_t b = 0; b < in->n; b += (uint32_t)cap) {
        const size_t n = std::min<size_t>(cap, in->n - b);
        std::memcpy(ht, in->tuple + 4u * b, n * 16);
        if (in->macs) std::memcpy(hm, in->macs + 4u * b, n * 16);
        if (in->ts) std::memcpy(hts, in->ts + b, n * 8);
        uint8_t *d = L.d;
        ppe_tuples_t dv = {(const uint32_t *)d, in->macs ? (const uint32_t *)(d + cap * 16) : nullptr,
                           in->ts ? (const uint64_t *)(d + cap * 32) : nullptr, (uint32_t)n};
        int rc = ppe_acl_lookup(c, &dv, (int32_t *)(d + cap * 40), (uint32_t *)(d + cap * 44), now_seconds, L.s);
        if (rc != PPE_OK) return rc;
        // spin on this stream alone (a lookup is a few microseconds; a blocking wait would add the wake-up), then
        // block
        hipError_t q = hipErrorNotReady;
        const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        while ((q = hipStreamQuery(L.s)) == hipErrorNotReady && std::chrono::steady_clock::now() < until)
            __builtin_ia32_pause();
        if (q == hipErrorNotReady) q = hipStreamSynchronize(L.s);
        if (q != hipSuccess) return fail(c, PPE_EIO, "acl lookup kernel failed: %s", hipGetErrorString(q));
        if (hit) std::memcpy(hit + b, hh, n * 4);
        if (action) std::memcpy(action + b, ha, n * 4);
    }
    return PPE_OK;
}

void *ppe_dev_alloc(ppe_ctx_t *c, size_t bytes) {
    void *p = nullptr;
    if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return p;
}
void ppe_dev_free(ppe_ctx_t *c, void *p) {
    if (c && p && hipSetDevice(c->device) == hipSuccess) (void)hipFree(p);
}
void *ppe_host_alloc(ppe_ctx_t *c, size_t bytes) {
    void *p = nullptr;
    if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void ppe_host_free(ppe_ctx_t *c, void *p) {
    if (c && p) (void)hipHostFree(p);
}
int ppe_memcpy_h2d(ppe_ctx_t *c, void *dst, const void *src, size_t bytes) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PPE_OK;
}
int ppe_memcpy_d2h(ppe_ctx_t *c, void *dst, const void *src, size_t bytes) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PPE_OK;
}
int ppe_memset_d(ppe_ctx_t *c, void *dst, int value, size_t bytes) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemset(dst, value, bytes));
    return PPE_OK;
}
int ppe_sync(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    return PPE_OK;
}

int ppe_counters_read(ppe_ctx_t *c, ppe_counters_t *out) {
    if (!c || !out) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t words = (size_t)kSlotSets * c->max_grid * PPE_CSLOT_WORDS;
    std::vector<unsigned long long> h(words);
    HIPCHK(c, hipMemcpy(h.data(), c->d_cslots, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    for (size_t b = 0; b < (size_t)kSlotSets * c->max_grid; ++b)
        for (int i = 0; i < PPE_CSLOT_WORDS; ++i) out->c[i] += h[b * PPE_CSLOT_WORDS + i];
    return PPE_OK;
}

int ppe_counters_clear(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemset(c->d_cslots, 0,
                        (size_t)kSlotSets * c->max_grid * PPE_CSLOT_WORDS * sizeof(unsigned long long)));
    return PPE_OK;
}

int ppe_stream_tcp_set(ppe_ctx_t *c, const ppe_stream_tcp_cfg_t *cfg) {
    if (!c) return PPE_EINVAL;
    const ppe_stream_tcp_cfg_t ref = {1u, 0u, 0u, 1u};  // stream-tcp.c:16-21
    const ppe_stream_tcp_cfg_t v = cfg ? *cfg : ref;
    if (v.track > 1 || v.midstream > 1 || v.async_oneside > 1 || v.reasm > 1)
        return fail(c, PPE_EINVAL, "ppe_stream_tcp_set: every word must be 0/1");
    // sessions attached and tracking goes on: flows alive now have no session (ssn == NULL), every record zero
    if (c->flow && c->flow->stream_on && !c->stcp.track && v.track) {
        const int rc = flow_stream_zero(c);
        if (rc != PPE_OK) return rc;
    }
    c->stcp = v;  // by value into the kernel arguments of later launches
    return PPE_OK;
}

int ppe_stream_tcp_get(ppe_ctx_t *c, ppe_stream_tcp_cfg_t *cfg) {
    if (!c || !cfg) return PPE_EINVAL;
    *cfg = c->stcp;
    return PPE_OK;
}

int ppe_stream_counters_read(ppe_ctx_t *c, ppe_stream_counters_t *out) {
    if (!c || !out) return PPE_EINVAL;
    static_assert(PPE_SSLOT_WORDS == PPE_SC__COUNT && PPE_SC__COUNT <= 16, "stream counter slots");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t words = (size_t)kSlotSets * c->max_grid * PPE_SSLOT_WORDS;
    std::vector<unsigned long long> h(words);
    HIPCHK(c, hipMemcpy(h.data(), c->d_sslots, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    for (size_t b = 0; b < (size_t)kSlotSets * c->max_grid; ++b)
        for (int i = 0; i < PPE_SSLOT_WORDS; ++i) out->c[i] += h[b * PPE_SSLOT_WORDS + i];
    return PPE_OK;
}

int ppe_stream_counters_clear(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemset(c->d_sslots, 0,
                        (size_t)kSlotSets * c->max_grid * PPE_SSLOT_WORDS * sizeof(unsigned long long)));
    return PPE_OK;
}

// ---- port-scan detector (dataplane/src/attack/dp_portscan.c) ----
static void ps_free(ppe_portscan_table *t) {
    void *ptrs[] = {t->keys, t->recs, t->ctl, t->slot_of, t->dport, t->cbase, t->work, t->pts, t->skey, t->cmask,
                    t->mask, t->res};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete t;
}

static int ps_check_words(const ppe_portscan_cfg_t &v) { return (v.able > 1u || v.action > 1u) ? PPE_EINVAL : PPE_OK; }

int ppe_portscan_create(ppe_ctx_t *c, const ppe_portscan_cfg_t *cfg, ppe_portscan_t **out) {
    if (!c || !out) return PPE_EINVAL;
    *out = nullptr;
    // portscan_able 1, portscan_action 0, portscan_exception_freq 50 (dp_portscan.c:9-11), flood_hold_time 600
    // (dp_attack.c:25)
    ppe_portscan_cfg_t v = {1u, 0u, 50u, 600u, 0u, 0u, 0u, 0u};
    if (cfg) v = *cfg;
    if (ps_check_words(v) != PPE_OK) return fail(c, PPE_EINVAL, "ppe_portscan_create: able and action must be 0/1");
    if (v.capacity == 0) v.capacity = 100000u;  // PORTSCAN_ITEM_NUM (dp_portscan.h:67)
    if (v.max_batch == 0) v.max_batch = 1u << 20;
    if (v.cycles_per_second == 0) v.cycles_per_second = 1000000000ull;
    v.pad = 0;
    if (v.capacity > (1u << 28) || v.max_batch > (1u << 28))
        return fail(c, PPE_EINVAL, "ppe_portscan_create: capacity / max_batch too large");
    HIPCHK(c, hipSetDevice(c->device));
    ppe_portscan_table *t = new ppe_portscan_table;
    t->ctx = c;
    t->cfg = v;
    t->fused_ok = env_int("PPE_PS_FUSED", 1) != 0;  // A/B switch: 0 keeps every batch on the staged launches
    uint32_t ns = 1024;
    while (ns < 2u * (v.capacity + v.max_batch)) ns <<= 1;
    t->nslots = ns;
    uint32_t npad = PPE_PS_SORT_BLOCK;
    while (npad < v.max_batch) npad <<= 1;
    t->npad_max = npad;
    const size_t m = v.max_batch, tiles = (m + 63u) / 64u;
    bool ok = hipMalloc(&t->keys, (size_t)ns * 8u) == hipSuccess &&
              hipMalloc(&t->recs, (size_t)ns * 8u * PPE_PS_REC_WORDS) == hipSuccess &&
              hipMalloc(&t->ctl, PPE_PSC_WORDS * 8u) == hipSuccess && hipMalloc(&t->slot_of, m * 4u) == hipSuccess &&
              hipMalloc(&t->dport, m * 4u) == hipSuccess && hipMalloc(&t->cbase, tiles * 4u) == hipSuccess &&
              hipMalloc(&t->work, m * 4u) == hipSuccess && hipMalloc(&t->pts, m * 8u) == hipSuccess &&
              hipMalloc(&t->skey, (size_t)npad * 8u) == hipSuccess && hipMalloc(&t->cmask, tiles * 8u) == hipSuccess &&
              hipMalloc(&t->mask, tiles * 8u) == hipSuccess && hipMalloc(&t->res, m) == hipSuccess;
    t->mask_cap = ok ? tiles : 0;
    ok = ok && hipMemset(t->keys, 0, (size_t)ns * 8u) == hipSuccess &&
         hipMemset(t->recs, 0, (size_t)ns * 8u * PPE_PS_REC_WORDS) == hipSuccess &&
         hipMemset(t->ctl, 0, PPE_PSC_WORDS * 8u) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ps_free(t);
        return fail(c, PPE_ENOMEM, "ppe_portscan_create: out of device memory");
    }
    *out = t;
    return PPE_OK;
}

int ppe_portscan_destroy(ppe_portscan_t *t) {
    if (!t) return PPE_EINVAL;
    (void)hipSetDevice(t->ctx->device);
    (void)hipDeviceSynchronize();
    if (t->ctx->ps == t) t->ctx->ps = nullptr;
    if (t->ctx->ps_flow == t) t->ctx->ps_flow = nullptr;
    ps_free(t);
    return PPE_OK;
}

int ppe_portscan_attach(ppe_ctx_t *c, ppe_portscan_t *t) {
    if (!c) return PPE_EINVAL;
    if (t && t->ctx != c) return fail(c, PPE_EINVAL, "ppe_portscan_attach: the table belongs to another context");
    if (t && c->ps_flow == t)
        return fail(c, PPE_EINVAL, "ppe_portscan_attach: the table is attached with ppe_flow_portscan_attach: detach first");
    c->ps = t;
    return PPE_OK;
}

// The flow-table path's attachment point: the same table and detector, called on flow misses only (flow.c:196-230), so
// a table runs under one of the two
int ppe_flow_portscan_attach(ppe_ctx_t *c, ppe_portscan_t *t) {
    if (!c) return PPE_EINVAL;
    if (t && t->ctx != c) return fail(c, PPE_EINVAL, "ppe_flow_portscan_attach: the table belongs to another context");
    if (t && c->ps == t)
        return fail(c, PPE_EINVAL, "ppe_flow_portscan_attach: the table is attached with ppe_portscan_attach: detach first");
    c->ps_flow = t;
    return PPE_OK;
}

uint32_t ppe_flow_portscan_max(void) { return PPE_FLOW_PS_MAX; }

// The context's switch for a port-scan table (able 1) and attack monitors both flow-attached: off, ppe_classify_flow
// refuses such a batch, as it always did; on, it runs the monitors, the detector and the table in one launch
// (ppe_pick_flow_combined).  Like the attachments it is the context's: ppe_flow_destroy leaves it
int ppe_flow_combine(ppe_ctx_t *c, uint32_t on) {
    if (!c) return PPE_EINVAL;
    if (on > 1u) return fail(c, PPE_EINVAL, "ppe_flow_combine: on must be 0 or 1");
    c->flow_combine = on;
    return PPE_OK;
}

int ppe_portscan_clock(ppe_portscan_t *t, uint64_t now_cycles, uint64_t now_seconds) {
    if (!t) return PPE_EINVAL;
    t->now_cycles = now_cycles;  // by value into the kernel arguments of the batches enqueued from now on
    t->now_seconds = now_seconds;
    return PPE_OK;
}

int ppe_portscan_set(ppe_portscan_t *t, const ppe_portscan_cfg_t *cfg) {
    if (!t || !cfg) return PPE_EINVAL;
    if (ps_check_words(*cfg) != PPE_OK) return ps_fail(t, PPE_EINVAL, "ppe_portscan_set: able and action must be 0/1");
    t->cfg.able = cfg->able;                      // dp_portscan_able_set, dp_cmd.c:2141-2145
    t->cfg.action = cfg->action;                  // dp_portscan_action_set, :2203-2207
    t->cfg.exception_freq = cfg->exception_freq;  // dp_portscan_freq_set, :2239-2243
    t->cfg.hold_seconds = cfg->hold_seconds;      // flood_hold_time, :2225
    return PPE_OK;
}

int ppe_portscan_age(ppe_portscan_t *t, uint64_t now_cycles, uint64_t *freed) {
    if (!t) return PPE_EINVAL;
    PSCHK(t, hipSetDevice(t->ctx->device));
    PSCHK(t, hipDeviceSynchronize());
    unsigned long long d0 = 0, d1 = 0;
    PSCHK(t, hipMemcpy(&d0, t->ctl + PPE_PSC_DEL, 8, hipMemcpyDeviceToHost));
    const int rc = ps_rebuild(t, 1, now_cycles);
    if (rc != PPE_OK) return rc;
    PSCHK(t, hipMemcpy(&d1, t->ctl + PPE_PSC_DEL, 8, hipMemcpyDeviceToHost));
    if (freed) *freed = d1 - d0;
    return PPE_OK;
}

int ppe_portscan_info(ppe_portscan_t *t, ppe_portscan_info_t *info) {
    if (!t || !info) return PPE_EINVAL;
    PSCHK(t, hipSetDevice(t->ctx->device));
    PSCHK(t, hipDeviceSynchronize());
    unsigned long long h[PPE_PSC_WORDS];
    PSCHK(t, hipMemcpy(h, t->ctl, sizeof h, hipMemcpyDeviceToHost));
    std::memset(info, 0, sizeof *info);
    info->live = h[PPE_PSC_LIVE];
    info->new_pcb = h[PPE_PSC_NEW];
    info->del_pcb = h[PPE_PSC_DEL];
    info->ok = h[PPE_PSC_OK];
    info->nomem = h[PPE_PSC_NOMEM];
    info->detected = h[PPE_PSC_DETECTED];
    info->hold = h[PPE_PSC_HOLD];
    info->drop = h[PPE_PSC_DROP];
    info->cfg = t->cfg;
    info->slots = t->nslots;
    info->rebuilds = t->rebuilds;
    return PPE_OK;
}

int ppe_portscan_dump(ppe_portscan_t *t, ppe_portscan_entry_t *entries, uint32_t max, uint32_t *n) {
    if (!t || !n || (max && !entries)) return PPE_EINVAL;
    PSCHK(t, hipSetDevice(t->ctx->device));
    PSCHK(t, hipDeviceSynchronize());
    std::vector<unsigned long long> k(t->nslots), r((size_t)t->nslots * PPE_PS_REC_WORDS);
    PSCHK(t, hipMemcpy(k.data(), t->keys, k.size() * 8u, hipMemcpyDeviceToHost));
    PSCHK(t, hipMemcpy(r.data(), t->recs, r.size() * 8u, hipMemcpyDeviceToHost));
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < t->nslots; ++s) {
        const unsigned long long *q = &r[(size_t)s * PPE_PS_REC_WORDS];
        if (k[s] == 0 || !((uint32_t)q[4] & PPE_PS_LIVE)) continue;
        if (cnt < max) {
            ppe_portscan_entry_t &e = entries[cnt];
            e.sip = (uint32_t)k[s];
            e.last_dport = (uint32_t)q[4] & 0xffffu;
            e.exception = (uint32_t)q[3];
            e.last_exception = (uint32_t)(q[3] >> 32);
            e.last_cycle = q[0];
            e.cycle = q[1];
            e.hold = q[2];
        }
        ++cnt;
    }
    *n = cnt;
    return PPE_OK;
}

int ppe_portscan_prepass_info(ppe_portscan_t *t, uint32_t *kind, uint32_t *launches) {
    if (!t) return PPE_EINVAL;
    if (kind) *kind = t->last_kind;
    if (launches) *launches = t->last_launches;
    return PPE_OK;
}

const char *ppe_portscan_last_error(ppe_portscan_t *t) { return t ? t->err : "null port-scan table"; }

// ---- attack monitors (dataplane/src/attack/dp_attack.c) ----
static int atk_fail(ppe_attack *t, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t->err, sizeof t->err, fmt, ap);
    va_end(ap);
    if (t->ctx) std::snprintf(t->ctx->err, sizeof t->ctx->err, "%s", t->err);
    return code;
}
#define ATKCHK(t, expr)                                                                               \
    do {                                                                                              \
        hipError_t e_ = (hipError_t)(expr);                                                           \
        if (e_ != hipSuccess) return atk_fail((t), PPE_EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// all = true: after a device synchronise; else only the tables whose event has completed
static void atk_free_retired(ppe_attack *t, bool all) {
    size_t keep = 0;
    for (auto &r : t->retired) {
        if (all || !r.done || hipEventQuery(r.done) == hipSuccess) {
            (void)hipFree(r.p);
            if (r.done) (void)hipEventDestroy(r.done);
        } else {
            t->retired[keep++] = r;
        }
    }
    t->retired.resize(keep);
    (void)hipGetLastError();  // (hipErrorNotReady of a pending event is no error of the caller's)
}

// the rules reduced to what the monitors read; every test of the reference is == ATTACK_ENABLE (1)
static void atk_rule_args(const ppe_attack_cfg_t &v, ppe_atk_kargs &a) {
    for (int p = 0; p < PPE_ATTACK_PORTS; ++p) {
        const ppe_attack_pd_t &pd = v.pd[p];
        const ppe_attack_td_t &td = v.td[p];
        a.rule[p][0] = ((pd.land == 1u && pd.drop_pack == 1u) ? PPE_ATK_EN_LAND : 0u) |
                       ((td.flood_udp == 1u && td.drop_pack == 1u) ? PPE_ATK_EN_UDP : 0u) |
                       ((td.flood_syn == 1u && td.drop_pack == 1u) ? PPE_ATK_EN_SYN : 0u) |
                       (td.drop_pack == 1u ? PPE_ATK_EN_DROP : 0u);
        a.rule[p][1] = td.udp_speed;
        a.rule[p][2] = td.syn_speed;
        a.rule[p][3] = td.syn_count;
    }
}

int ppe_attack_create(ppe_ctx_t *c, const ppe_attack_cfg_t *cfg, ppe_attack_t **out) {
    if (!c || !out) return PPE_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    ppe_attack *t = new ppe_attack;
    t->ctx = c;
    if (cfg) t->cfg = *cfg;
    else t->cfg.hold_seconds = 600u;  // flood_hold_time (dp_attack.c:25); the rules all zero (DP_Attack_Del_All)
    t->cfg.pad = 0;
    ppe_atk_kargs a;
    std::memset(&a, 0, sizeof a);
    atk_rule_args(t->cfg, a);
    a.op = PPE_ATK_K_SET;
    const size_t slot_bytes = (size_t)c->max_grid * PPE_ATK_SLOT_WORDS * 8u;
    bool ok = hipMalloc(&t->d_st, PPE_ATK_WORDS * 8u) == hipSuccess &&
              hipMemset(t->d_st, 0, PPE_ATK_WORDS * 8u) == hipSuccess && hipMalloc(&t->d_slots, slot_bytes) == hipSuccess &&
              hipMemset(t->d_slots, 0, slot_bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    a.st = t->d_st;
    ok = ok && ppe_launch_attack_ctl(&a, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (t->d_st) (void)hipFree(t->d_st);
        if (t->d_slots) (void)hipFree(t->d_slots);
        delete t;
        return fail(c, PPE_ENOMEM, "ppe_attack_create: no device memory, or the first rule load failed");
    }
    *out = t;
    return PPE_OK;
}

int ppe_attack_destroy(ppe_attack_t *t) {
    if (!t) return PPE_EINVAL;
    (void)hipSetDevice(t->ctx->device);
    (void)hipDeviceSynchronize();
    if (t->ctx->atk == t) t->ctx->atk = nullptr;
    if (t->ctx->atk_flow == t) t->ctx->atk_flow = nullptr;
    atk_free_retired(t, true);
    if (t->d_ports) (void)hipFree((void *)t->d_ports);
    (void)hipFree(t->d_st);
    (void)hipFree(t->d_slots);
    delete t;
    return PPE_OK;
}

int ppe_attack_attach(ppe_ctx_t *c, ppe_attack_t *t) {
    if (!c) return PPE_EINVAL;
    if (t && t->ctx != c) return fail(c, PPE_EINVAL, "ppe_attack_attach: the object belongs to another context");
    if (t && c->atk_flow == t)
        return fail(c, PPE_EINVAL, "ppe_attack_attach: the object is attached with ppe_flow_attack_attach: detach first");
    c->atk = t;
    return PPE_OK;
}

// The flow-table path's attachment point: the same object and monitors, but syncount_accum counts the flows TCP SYN
// packets create (FlowAdd, flow.c:151-154) instead of every forwarded SYN, so an object runs under one of the two
int ppe_flow_attack_attach(ppe_ctx_t *c, ppe_attack_t *t) {
    if (!c) return PPE_EINVAL;
    if (t && t->ctx != c) return fail(c, PPE_EINVAL, "ppe_flow_attack_attach: the object belongs to another context");
    if (t && c->atk == t)
        return fail(c, PPE_EINVAL, "ppe_flow_attack_attach: the object is attached with ppe_attack_attach: detach first");
    c->atk_flow = t;
    return PPE_OK;
}

int ppe_attack_set(ppe_attack_t *t, const ppe_attack_cfg_t *cfg) {
    if (!t || !cfg) return PPE_EINVAL;
    ATKCHK(t, hipSetDevice(t->ctx->device));
    ppe_atk_kargs a;
    std::memset(&a, 0, sizeof a);
    atk_rule_args(*cfg, a);
    a.st = t->d_st;
    a.op = PPE_ATK_K_SET;
    ATKCHK(t, ppe_launch_attack_ctl(&a, t->stream));
    t->cfg = *cfg;  // hold_seconds travels by value with the launches enqueued from now on
    t->cfg.pad = 0;
    return PPE_OK;
}

int ppe_attack_clock(ppe_attack_t *t, uint64_t now_seconds) {
    if (!t) return PPE_EINVAL;
    t->now = now_seconds;
    return PPE_OK;
}

int ppe_attack_tick(ppe_attack_t *t, uint64_t now_seconds) {
    if (!t) return PPE_EINVAL;
    ATKCHK(t, hipSetDevice(t->ctx->device));
    ppe_atk_kargs a;
    std::memset(&a, 0, sizeof a);
    a.st = t->d_st;
    a.slots = t->d_slots;
    a.nslots = t->ctx->max_grid;
    a.op = PPE_ATK_K_TICK;
    a.now = now_seconds;
    ATKCHK(t, ppe_launch_attack_ctl(&a, t->stream));
    t->now = now_seconds;
    return PPE_OK;
}

int ppe_attack_ports(ppe_attack_t *t, const uint8_t *const *ports, uint32_t nbatch) {
    if (!t) return PPE_EINVAL;
    if (!ports) nbatch = 0;
    if (nbatch > PPE_MAX_RING) return atk_fail(t, PPE_EINVAL, "ppe_attack_ports: more than %d batches", PPE_MAX_RING);
    ATKCHK(t, hipSetDevice(t->ctx->device));
    // launches in flight may still read the table in use: it is retired, not rewritten
    const uint8_t **nt = nullptr;
    if (nbatch) {
        ATKCHK(t, hipMalloc(&nt, (size_t)nbatch * sizeof(*nt)));
        const hipError_t e = hipMemcpy((void *)nt, ports, (size_t)nbatch * sizeof(*nt), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree((void *)nt);
            return atk_fail(t, PPE_EIO, "ppe_attack_ports: %s", hipGetErrorString(e));
        }
    }
    if (t->d_ports) {
        // behind every launch enqueued so far on the classify stream; no event: kept until the next synchronise
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, t->stream) != hipSuccess) {
            if (ev) (void)hipEventDestroy(ev);
            ev = nullptr;
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
        }
        t->retired.push_back({(void *)t->d_ports, ev});
    }
    atk_free_retired(t, false);
    t->d_ports = nt;
    t->h_ports.assign(ports, ports + nbatch);
    return PPE_OK;
}

int ppe_attack_info(ppe_attack_t *t, ppe_attack_info_t *info) {
    if (!t || !info) return PPE_EINVAL;
    ATKCHK(t, hipSetDevice(t->ctx->device));
    ATKCHK(t, hipDeviceSynchronize());
    atk_free_retired(t, true);
    unsigned long long h[PPE_ATK_WORDS];
    ATKCHK(t, hipMemcpy(h, t->d_st, sizeof h, hipMemcpyDeviceToHost));
    // what the classify workgroups counted since the last tick is still in their slots
    std::vector<unsigned long long> sl((size_t)t->ctx->max_grid * PPE_ATK_SLOT_WORDS);
    ATKCHK(t, hipMemcpy(sl.data(), t->d_slots, sl.size() * 8u, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < t->ctx->max_grid; ++b) {
        const unsigned long long *q = &sl[b * PPE_ATK_SLOT_WORDS];
        for (int p = 0; p < PPE_ATTACK_PORTS; ++p) {
            unsigned long long *s = h + PPE_ATK_PORT0 + PPE_ATK_PORT_STRIDE * p;
            s[PPE_ATK_UDP_ACCUM] += q[3 * p];
            s[PPE_ATK_SYN_ACCUM] += q[3 * p + 1];
            s[PPE_ATK_SYNCNT_ACCUM] += q[3 * p + 2];
            h[PPE_ATK_TOTALS + p] += q[12 + p];
        }
    }
    std::memset(info, 0, sizeof *info);
    info->cfg = t->cfg;
    for (int p = 0; p < PPE_ATTACK_PORTS; ++p) {
        const unsigned long long *s = h + PPE_ATK_PORT0 + PPE_ATK_PORT_STRIDE * p;
        ppe_attack_port_t &o = info->ai[p];
        o.udppps = s[PPE_ATK_UDPPPS];
        o.udp_accum = s[PPE_ATK_UDP_ACCUM];
        o.synpps = s[PPE_ATK_SYNPPS];
        o.syn_accum = s[PPE_ATK_SYN_ACCUM];
        o.syncount = s[PPE_ATK_SYNCNT];
        o.syncount_accum = s[PPE_ATK_SYNCNT_ACCUM];
        o.syn_flood_hold = s[PPE_ATK_SYN_HOLD];
        o.syn_flood_hold_time = s[PPE_ATK_SYN_HOLD_TIME];
        o.udp_flood_hold = s[PPE_ATK_UDP_HOLD];
        o.udp_flood_hold_time = s[PPE_ATK_UDP_HOLD_TIME];
    }
    info->land_drop = h[PPE_ATK_TOTALS + 0];
    info->udpflood_drop = h[PPE_ATK_TOTALS + 1];
    info->synflood_drop = h[PPE_ATK_TOTALS + 2];
    info->syncount_drop = h[PPE_ATK_TOTALS + 3];
    info->now_seconds = t->now;
    return PPE_OK;
}

int ppe_attack_clear_stat(ppe_attack_t *t) {
    if (!t) return PPE_EINVAL;
    ATKCHK(t, hipSetDevice(t->ctx->device));
    ppe_atk_kargs a;
    std::memset(&a, 0, sizeof a);
    a.st = t->d_st;
    a.slots = t->d_slots;
    a.nslots = t->ctx->max_grid;
    a.op = PPE_ATK_K_CLEAR;
    ATKCHK(t, ppe_launch_attack_ctl(&a, t->stream));
    return PPE_OK;
}

const char *ppe_attack_last_error(ppe_attack_t *t) { return t ? t->err : "null attack object"; }

int ppe_timing_enable(ppe_ctx_t *c, int on) {
    if (!c) return PPE_EINVAL;
    c->timing = on != 0;
    return PPE_OK;
}

int ppe_timing_read(ppe_ctx_t *c, double *total_ms, uint32_t *launches, int reset) {
    if (!c) return PPE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    double t = 0;
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        HIPCHK(c, hipEventSynchronize(c->ev[i + 1]));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = (uint32_t)(c->ev_used / 2);
    if (reset) c->ev_used = 0;
    return PPE_OK;
}

int ppe_set_tuning(ppe_ctx_t *c, const ppe_tuning_t *t) {
    if (!c || !t) return PPE_EINVAL;
    if (t->block != 0 && t->block != 256 && t->block != 512 && t->block != 1024)
        return fail(c, PPE_EINVAL, "block must be 0 (auto), 256, 512 or 1024");
    if (t->pipeline != 0 && t->pipeline != 1 && t->pipeline != 3 && t->pipeline != 4 && t->pipeline != 5)
        return fail(c, PPE_EINVAL, "pipeline must be 0 (auto), 1 (first tile at the loop top), 3 (4 tiles per wave "
                                   "walking the block section together), 4 (first tile's loads before the image "
                                   "staging) or 5 (the cut lists of a v8 image)");
    if (t->blocks_per_cu > kMaxBlocksPerCU) return fail(c, PPE_EINVAL, "blocks_per_cu must be <= 32");
    if (t->batches_per_launch > PPE_MAX_RING) return fail(c, PPE_EINVAL, "batches_per_launch must be <= 4096");
    c->tune = *t;
    c->tune.pipeline = t->pipeline;
    c->tune.lds_image = t->lds_image ? 1u : 0u;
    for (int r = 0; r < 2; ++r)
        if (!c->h_img[r].empty()) {
            const int rc = plan_slot(c, r);
            if (rc != PPE_OK) return rc;
        }
    return PPE_OK;
}

int ppe_get_tuning(ppe_ctx_t *c, ppe_tuning_t *t) {
    if (!c || !t) return PPE_EINVAL;
    *t = c->tune;
    return PPE_OK;
}

int ppe_acl_image(ppe_ctx_t *c, uint32_t *words, uint32_t *n_words) {
    if (!c || !n_words) return PPE_EINVAL;
    const std::vector<uint32_t> &img = c->h_img[c->running];
    if (words) std::memcpy(words, img.data(), std::min<size_t>(*n_words, img.size()) * 4u);
    *n_words = (uint32_t)img.size();
    return PPE_OK;
}

int ppe_launch_info(ppe_ctx_t *c, uint32_t *grid, uint32_t *block, uint32_t *lds_bytes, uint32_t *variant) {
    if (!c) return PPE_EINVAL;
    const ppe_plan &plan = c->plan[c->running][0];
    if (grid) *grid = std::min(c->n_cu * blocks_per_cu(c, c->running), c->max_grid);
    if (block) *block = plan.block;
    if (lds_bytes) *lds_bytes = plan.lds_bytes;
    if (variant) *variant = plan.mode | (plan.pipe << 4);
    return PPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Flow table (FlowInit / FlowHandlePacket / FlowAgeTimeoutCB / FlowRelease, dataplane/src/flow/flow.c)

static void flow_free_arrays(FlowArrays &a) {
    (void)hipFree(a.keys);
    (void)hipFree(a.creator);
    (void)hipFree(a.stats);
    (void)hipFree(a.recs);
    (void)hipFree(a.sess);
    a = FlowArrays();
}

// allocate (if needed) and clear one slot-array set: every slot EMPTY with zero counters, no creator
static int flow_clear_arrays(ppe_ctx *c, FlowArrays &a, uint32_t nslots, hipStream_t s) {
    if (!a.keys) {
        if (hipMalloc(&a.keys, (size_t)nslots * 4u * PPE_FLOW_SLOT_WORDS) != hipSuccess ||
            hipMalloc(&a.recs, (size_t)nslots * 8u * PPE_FLOW_REC_WORDS) != hipSuccess ||
            hipMalloc(&a.creator, (size_t)nslots * 4u) != hipSuccess ||
            hipMalloc(&a.stats, (size_t)nslots * 32u) != hipSuccess) {
            flow_free_arrays(a);
            return fail(c, PPE_ENOMEM, "flow table: out of device memory (%u slots)", nslots);
        }
    }
    HIPCHK(c, hipMemsetAsync(a.keys, 0, (size_t)nslots * 4u * PPE_FLOW_SLOT_WORDS, s));
    HIPCHK(c, hipMemsetAsync(a.recs, 0, (size_t)nslots * 8u * PPE_FLOW_REC_WORDS, s));
    HIPCHK(c, hipMemsetAsync(a.creator, 0xff, (size_t)nslots * 4u, s));
    HIPCHK(c, hipMemsetAsync(a.stats, 0, (size_t)nslots * 32u, s));
    if (c->flow && c->flow->stream_on) {  // the session records beside them, every one zero
        if (!a.sess && hipMalloc(&a.sess, (size_t)nslots * 4u * PPE_FLOW_SESS_WORDS) != hipSuccess)
            return fail(c, PPE_ENOMEM, "flow table: out of device memory (%u session records)", nslots);
        HIPCHK(c, hipMemsetAsync(a.sess, 0, (size_t)nslots * 4u * PPE_FLOW_SESS_WORDS, s));
    }
    return PPE_OK;
}

// every session record of the slot arrays in use back to zero (synchronises: batches in flight finish first)
static int flow_stream_zero(ppe_ctx *c) {
    FlowTable &t = *c->flow;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (t.arr[t.cur].sess) HIPCHK(c, hipMemset(t.arr[t.cur].sess, 0, (size_t)t.nslots * 4u * PPE_FLOW_SESS_WORDS));
    return PPE_OK;
}

static ppe_flowdev flow_dev(const FlowTable &t, int which) {
    ppe_flowdev d;
    std::memset(&d, 0, sizeof d);
    const FlowArrays &a = t.arr[which];
    d.keys = a.keys;
    d.stats = a.stats;
    d.packed = a.recs;
    d.miss_tiles = t.miss_tiles;
    d.parity = (uint32_t)(t.batches & 1u);
    d.fold_pkts = t.fold_pkts;
    d.fold_bytes = t.fold_bytes;
    d.snap = t.snap_d;
    d.seq = t.batches;
    d.creator = a.creator;
    d.ctl = t.ctl;
    d.rec = t.rec;
    d.tile_miss = t.tile_miss;
    d.tile_new = t.tile_new;
    d.rslot = t.rslot;
    d.gmask = t.nslots / PPE_FLOW_GROUP - 1u;
    d.capacity = t.capacity;
    d.upd = t.upd;
    d.ucnt = t.ucnt;
    d.upd_wgs = t.upd_wgs;
    d.upd_osh = t.upd_osh;
    d.upd_owners = t.upd_owners;
    d.upd_hmask = t.upd_hmask;
    return d;
}

static uint32_t flow_grid(const ppe_ctx *c, uint64_t items, uint32_t per_wg) {
    const uint64_t want = (items + per_wg - 1u) / per_wg;
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(want, (uint64_t)c->n_cu * 8u));
}

// exact live / tombstone counts (synchronises)
// Tighten the host's live / tombstone bounds from the latest snapshot the classify launches publish in pinned memory
// (seqlock: the sequence word is written last and re-read here).
static void flow_apply_snapshot(FlowTable &t) {
    const volatile unsigned long long *sh = t.snap_h;
    const uint64_t s0 = sh[0], live = sh[1], tombs = sh[2], s1 = sh[0];
    if (s0 == s1 && s0 > t.snap_used && s0 <= t.batches && t.batches - s0 < FlowTable::kSnapRing) {
        t.snap_used = s0;
        t.live_ub = std::min<uint64_t>(live + (t.tot_n - t.cum_n[s0 % FlowTable::kSnapRing]), t.capacity);
        t.tomb_ub = tombs + (t.tot_rev - t.cum_rev[s0 % FlowTable::kSnapRing]);
    }
}

static int flow_sync_counts(ppe_ctx *c, unsigned long long *ctl_out) {
    FlowTable &t = *c->flow;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(ctl_out, t.ctl, PPE_FCTL_WORDS * 8u, hipMemcpyDeviceToHost));
    if (ctl_out[PPE_FCTL_ERR]) {
        // reported once: the word is cleared, so only this call fails (the batches it covers may be inexact; the
        // table itself stays usable)
        HIPCHK(c, hipMemset(t.ctl + PPE_FCTL_ERR, 0, 8u));
        HIPCHK(c, hipDeviceSynchronize());
        return fail(c, PPE_EIO, "flow table: %llu finalize workgroup(s) timed out waiting for the revoke", ctl_out[PPE_FCTL_ERR]);
    }
    t.live_ub = ctl_out[PPE_FCTL_LIVE];
    t.tomb_ub = ctl_out[PPE_FCTL_TOMBS];
    t.snap_used = t.batches;  // (the device is idle: this is the state after every submitted batch)
    return PPE_OK;
}

// Rebuild the table without tombstones when they exceed a quarter of the slots (keeps every probe sequence short
// and an EMPTY slot on each).  Synchronises when the host bound says it may be needed.
static int flow_maybe_rehash(ppe_ctx *c) {
    FlowTable &t = *c->flow;
    if (t.tomb_ub <= t.nslots / 4u) return PPE_OK;
    unsigned long long ctl[PPE_FCTL_WORDS];
    int rc = flow_sync_counts(c, ctl);
    if (rc != PPE_OK || t.tomb_ub <= t.nslots / 4u) return rc;
    const int dst = 1 - t.cur;
    rc = flow_clear_arrays(c, t.arr[dst], t.nslots, nullptr);
    if (rc != PPE_OK) return rc;
    ppe_flow_kargs k;
    std::memset(&k, 0, sizeof k);
    k.f = flow_dev(t, t.cur);
    k.dst = flow_dev(t, dst);
    k.nslots = t.nslots;
    rc = ppe_launch_flow(PPE_FLOW_K_REHASH, &k, flow_grid(c, t.nslots, 256u), nullptr);
    if (rc != 0) return fail(c, PPE_EIO, "flow rehash launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (t.stream_on) {  // the session records follow their flows: a pass of its own behind the rehash launch
        ppe_flow_st_rehash_kargs sk;
        std::memset(&sk, 0, sizeof sk);
        sk.src_keys = t.arr[t.cur].keys;
        sk.dst_keys = t.arr[dst].keys;
        sk.src_sess = t.arr[t.cur].sess;
        sk.dst_sess = t.arr[dst].sess;
        sk.nslots = t.nslots;
        sk.dst_gmask = t.nslots / PPE_FLOW_GROUP - 1u;
        rc = ppe_launch_flow_stream_rehash(&sk, flow_grid(c, t.nslots, 256u), nullptr);
        if (rc != 0) return fail(c, PPE_EIO, "flow session rehash launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    HIPCHK(c, hipMemset(t.ctl + PPE_FCTL_TOMBS, 0, 8u));
    HIPCHK(c, hipDeviceSynchronize());
    t.cur = dst;
    t.tomb_ub = 0;
    ++t.rehashes;
    return PPE_OK;
}

// Test hook (tests/test_gpu_flow.py only, not in the public headers): the next `k` post-classify launches of
// ppe_classify_flow fail as a launch error would, after the batch's classify launch has run.
static uint32_t g_fail_post = 0;
extern "C" void ppe_flow_debug_fail_post(uint32_t k) { __atomic_store_n(&g_fail_post, k, __ATOMIC_RELAXED); }
static bool take_fail_post() {
    uint32_t k = __atomic_load_n(&g_fail_post, __ATOMIC_RELAXED);
    while (k)
        if (__atomic_compare_exchange_n(&g_fail_post, &k, k - 1, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return true;
    return false;
}

// the table exists and no batch was left half-done by a failed post-classify launch
static int flow_usable(ppe_ctx *c) {
    if (!c->flow) return fail(c, PPE_EINVAL, "no flow table (ppe_flow_create)");
    if (c->flow->broken)
        return fail(c, PPE_EIO, "flow table unusable: a batch's post-classify launch failed (ppe_flow_destroy it)");
    return PPE_OK;
}

int ppe_flow_destroy(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    if (!c->flow) return PPE_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    FlowTable *t = c->flow;
    for (FlowArrays &a : t->arr) flow_free_arrays(a);
    if (t->snap_h) (void)hipHostFree(t->snap_h);
    if (t->pre_launch) (void)hipEventDestroy(t->pre_launch);
    (void)hipFree(t->ctl);
    (void)hipFree(t->rec);
    (void)hipFree(t->rslot);
    (void)hipFree(t->miss_tiles);
    (void)hipFree(t->tile_miss);
    (void)hipFree(t->tile_new);
    (void)hipFree(t->upd);
    (void)hipFree(t->ucnt);
    (void)hipFree(t->tuple_scr);
    delete t;
    c->flow = nullptr;
    return PPE_OK;
}

int ppe_flow_create(ppe_ctx_t *c, uint32_t capacity, uint32_t max_batch) {
    if (!c) return PPE_EINVAL;
    if (capacity == 0) capacity = 100000u;  // MEM_POOL_FLOW_NODE_NUM, dataplane/src/platform/mem_pool.h:72
    if (max_batch == 0) max_batch = 1u << 20;
    if (capacity > (1u << 26) || max_batch > (1u << 26))
        return fail(c, PPE_EINVAL, "flow table: capacity and max_batch must be <= 2^26");
    HIPCHK(c, hipSetDevice(c->device));
    ppe_flow_destroy(c);
    FlowTable *t = new (std::nothrow) FlowTable();
    if (!t) return PPE_ENOMEM;
    c->flow = t;
    t->capacity = capacity;
    t->max_batch = max_batch;
    t->use_event = env_int("PPE_FLOW_EVENT", 0) != 0;
    t->small_allowed = env_int("PPE_FLOW_SMALL", 1) != 0;
    // finalize on half the CUs: the update workgroups (one per CU by their LDS) start on the other half at once
    // (F1 batch 67.1 -> 66.3 µs against one per CU, 69.3 / 71.9 at 64 / 32: profiles/r5_ab_runs.md r5aq)
    t->fin_cap = (uint32_t)std::max(0, env_int("PPE_FLOW_FIN_WGS", (int)std::max(1u, c->n_cu / 2u)));
    // test hook: lower fold thresholds so the fold path runs on small inputs (values <= the defaults only)
    const int fp = env_int("PPE_FLOW_FOLD_PKTS", 0), fb = env_int("PPE_FLOW_FOLD_BYTES", 0);
    if (fp > 0 && (unsigned long long)fp < t->fold_pkts) t->fold_pkts = (unsigned long long)fp;
    if (fb > 0 && (unsigned long long)fb < t->fold_bytes) t->fold_bytes = (unsigned long long)fb;
    // load <= 1/2 with the pool full and a whole batch of claims pending; tombstones are rehashed away at 1/4
    uint32_t ns = 64;
    while ((uint64_t)ns < 2ull * ((uint64_t)capacity + max_batch)) ns <<= 1;
    t->nslots = ns;
    const uint32_t tiles = (max_batch + 63u) / 64u;
    int rc = PPE_OK;
    if (hipMalloc(&t->ctl, PPE_FCTL_WORDS * 8u) != hipSuccess || hipMalloc(&t->rec, (size_t)max_batch * 16u) != hipSuccess ||
        hipMalloc(&t->rslot, (size_t)max_batch * 4u) != hipSuccess ||
        hipMalloc(&t->miss_tiles, (size_t)tiles * 4u) != hipSuccess ||
        hipMalloc(&t->tile_miss, (size_t)tiles * 8u) != hipSuccess ||
        hipMalloc(&t->tile_new, (size_t)tiles * 8u) != hipSuccess)
        rc = fail(c, PPE_ENOMEM, "flow table: out of device memory");
    if (rc == PPE_OK && hipMemset(t->ctl, 0, PPE_FCTL_WORDS * 8u) != hipSuccess) rc = fail(c, PPE_EIO, "memset");
    // owner-computed FlowUpdate: one bucket column per classify workgroup of a flow launch (at most 8 per CU and one
    // per 4 tiles of the largest batch; a workgroup past the columns updates its found flows by atomics);
    // PPE_FLOW_OWNER=0 turns it off (A/B)
    if (rc == PPE_OK && env_int("PPE_FLOW_OWNER", 1) != 0) {
        uint32_t owners = std::min<uint32_t>(PPE_UPD_OWNERS, ns), osh = 0;
        while ((ns >> osh) > owners) ++osh;
        t->upd_osh = osh;
        t->upd_owners = ns >> osh;
        t->upd_wgs = std::max(1u, std::min(c->n_cu * 8u, (tiles + 3u) / 4u));
        // test hook: a smaller LDS hash, so the update kernel's full-hash path runs on small inputs (power of two)
        const int hl = env_int("PPE_FLOW_UPD_HASH", 0);
        if (hl > 0 && hl < (int)PPE_UPD_HASH && (hl & (hl - 1)) == 0) t->upd_hmask = (uint32_t)hl - 1u;
        if (hipMalloc(&t->upd, (size_t)t->upd_owners * t->upd_wgs * PPE_UPD_CAP * 8u) != hipSuccess ||
            hipMalloc(&t->ucnt, (size_t)t->upd_owners * t->upd_wgs * 4u) != hipSuccess)
            rc = fail(c, PPE_ENOMEM, "flow table: out of device memory (update buckets)");
    }
    if (rc == PPE_OK && (hipHostMalloc(&t->snap_h, 64, hipHostMallocMapped) != hipSuccess ||
                         hipHostGetDevicePointer((void **)&t->snap_d, t->snap_h, 0) != hipSuccess))
        rc = fail(c, PPE_ENOMEM, "flow table: pinned snapshot buffer");
    if (rc == PPE_OK) std::memset(t->snap_h, 0, 64);
    if (rc == PPE_OK &&
        hipEventCreateWithFlags(&t->pre_launch, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess)
        rc = fail(c, PPE_EIO, "flow table: event");
    t->cum_n.assign(FlowTable::kSnapRing, 0);
    t->cum_rev.assign(FlowTable::kSnapRing, 0);
    if (rc == PPE_OK) rc = flow_clear_arrays(c, t->arr[0], ns, nullptr);
    if (rc == PPE_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(c, PPE_EIO, "flow table init failed");
    if (rc != PPE_OK) ppe_flow_destroy(c);
    return rc;
}

// how a flow batch of n packets runs with respect to the TCP session machine (ppe_pick_flow_stream_portscan over the
// context: ppe_pick_flow_stream's answer unless ppe_flow_stream_monitors or ppe_flow_stream_portscan is on)
static uint32_t flow_stream_pick(const ppe_ctx *c, uint32_t n) {
    return ppe_pick_flow_stream_portscan(n, c->flow && c->flow->stream_on, c->stcp.track, c->stcp.midstream,
                                         c->stcp.async_oneside, c->stcp.reasm, c->ps_flow != nullptr,
                                         c->atk_flow != nullptr, c->flow_st_monitors,
                                         c->ps_flow ? c->ps_flow->cfg.able : 0u, c->flow_st_portscan, c->flow_combine);
}
// (the planner's answers that are the session kernel with more inside: the session batch's checks and bookkeeping)
static bool fst_has_ps(uint32_t r) { return r == PPE_FST_KERNEL_PS || r == PPE_FST_KERNEL_PS_ATK; }
static bool fst_has_atk(uint32_t r) { return r == PPE_FST_KERNEL_ATK || r == PPE_FST_KERNEL_PS_ATK; }
// PPE_FST_REFUSE's error, by its cause
static int flow_stream_refuse(ppe_ctx *c) {
    if (c->stcp.midstream || c->stcp.async_oneside || c->stcp.reasm)
        return fail(c, PPE_ENOTSUP, "TCP sessions on the flow path are built for midstream 0, async_oneside 0, reasm 0 "
                                    "(ppe_stream_tcp_set)");
    // (ppe_flow_stream_portscan on and the combination itself runs, at one packet: the batch is what is refused)
    const bool size_only = c->flow_st_portscan == 1u && c->ps_flow && flow_stream_pick(c, 1u) != PPE_FST_REFUSE;
    if ((c->ps_flow || c->atk_flow) && !size_only)
        return fail(c, PPE_ENOTSUP, "TCP sessions on the flow path with a port-scan table or attack monitors flow-attached "
                                    "are not supported");
    // (with monitors flow-attached ppe_classify_flow_host is itself refused: the ports call is the one that chunks)
    if (size_only && c->atk_flow)
        return fail(c, PPE_ENOTSUP, "ppe_classify_flow with TCP sessions takes at most %u packets per batch "
                                    "(ppe_flow_stream_max; ppe_classify_flow_host_ports chunks larger ones)", PPE_FLOW_ST_MAX);
    return fail(c, PPE_ENOTSUP, "ppe_classify_flow with TCP sessions takes at most %u packets per batch "
                                "(ppe_flow_stream_max; ppe_classify_flow_host chunks larger ones)", PPE_FLOW_ST_MAX);
}

// ppe_classify_flow's body.  atk_pb: the port bytes the flow-attached monitors read (device pointer, or NULL: port 0);
// ports_call: the batch is a chunk of ppe_classify_flow_host_ports, which alone may take the one-launch kernel with the
// monitors in it (kind 4: ppe_classify_flow's own two launches with monitors attached are pinned by its tests)
static int classify_flow_run(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                             void *stream, const uint8_t *atk_pb, bool ports_call) {
    if (!c || !out) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    if (!out->verdict) return fail(c, PPE_EINVAL, "ppe_classify_flow needs the verdict output");
    // later packets of a tracked flow need the TCP session state machine (stream-tcp.c:3005-3140): that takes
    // ppe_flow_stream_attach, in the one configuration it is built for; refused before anything is touched otherwise
    const uint32_t fstm = flow_stream_pick(c, in ? in->n : 0u);
    // (the session kernel with the monitors in it, ppe_flow_stream_monitors, with the detector in it,
    // ppe_flow_stream_portscan, or both: the session batch's checks and bookkeeping)
    const bool fst_atk = fst_has_atk(fstm), fst_ps = fst_has_ps(fstm);
    const uint32_t fst = (fst_atk || fst_ps) ? (uint32_t)PPE_FST_KERNEL : fstm;
    if (c->stcp.track && fst == PPE_FST_PLAIN)
        return fail(c, PPE_ENOTSUP, "ppe_classify_flow with stream tracking on is not supported");
    if (fst == PPE_FST_REFUSE) return flow_stream_refuse(c);
    // PortScan_Detect runs on flow misses only (flow.c:196-215): a table attached for the stateless path would see every
    // packet; the flow path's detector takes ppe_flow_portscan_attach
    if (c->ps) return fail(c, PPE_ENOTSUP, "ppe_classify_flow with a port-scan table attached is not supported");
    // an object attached for the stateless path counts every forwarded SYN in syncount_accum; here it counts flow
    // creations (FlowAdd): that takes ppe_flow_attack_attach
    if (c->atk) return fail(c, PPE_ENOTSUP, "ppe_classify_flow with attack monitors attached is not supported");
    int rc = check_batch(c, in, cfg);
    if (rc != PPE_OK || in->n == 0) return rc;
    FlowTable &t = *c->flow;
    if (in->n > t.max_batch) return fail(c, PPE_EINVAL, "batch larger than the flow table's max_batch");
    // a SYN's window scale must lie inside the header window: neither PPE_ST_WINDOW_PUNT nor PPE_TUPLE_OPT_PAST between
    // a SYN and its option (Ethernet + VLAN + 60 + 60 B)
    if (fst == PPE_FST_KERNEL && in->stride < PPE_FLOW_STREAM_MIN_STRIDE)
        return fail(c, PPE_EINVAL, "ppe_classify_flow with TCP sessions needs a header stride of at least %u B",
                    PPE_FLOW_STREAM_MIN_STRIDE);
    // the detector on flow misses (a table flow-attached, portscan_able 1): one launch of one workgroup, up to
    // PPE_FLOW_PS_MAX packets; refused before anything is touched otherwise
    ppe_portscan_table *pt = c->ps_flow;
    const uint32_t fps = ppe_pick_flow_portscan(in->n, pt != nullptr, pt ? pt->cfg.able : 0u);
    // with monitors flow-attached as well: the kernel with both inside for a context that asked for it
    // (ppe_flow_combine), else refused
    const uint32_t fpc = ppe_pick_flow_combined(fps, c->atk_flow != nullptr, c->flow_combine);
    if (fps != PPE_FPS_PLAIN) {
        if (fpc == PPE_FPC_REFUSE && !c->flow_combine)
            return fail(c, PPE_ENOTSUP, "ppe_classify_flow with a port-scan table and attack monitors both flow-attached "
                                        "is not supported");
        if (fps == PPE_FPS_REFUSE)
            return fail(c, PPE_ENOTSUP, "ppe_classify_flow with a port-scan table flow-attached takes at most %u packets "
                                        "per batch (ppe_flow_portscan_max; ppe_classify_flow_host chunks larger ones)",
                        PPE_FLOW_PS_MAX);
        if (in->n > pt->cfg.max_batch)
            return fail(c, PPE_EINVAL, "batch of %u packets exceeds the port-scan table's max_batch %u", in->n,
                        pt->cfg.max_batch);
    }
    HIPCHK(c, use_device(c));
    flow_apply_snapshot(t);
    if (t.tomb_ub > t.nslots / 4u && t.snap_used + 1u < t.batches) {
        // The tombstone bound counts every packet of every batch since the snapshot as a possible revocation, so with
        // the host several batches ahead it passes the rehash threshold long before the table does.  Wait (bounded)
        // for the latest submitted batch's classify launch to publish its snapshot — one batch stays in flight, the
        // queue does not drain — and decide on that tighter bound before synchronising.  The host polls the snapshot
        // the launch's first workgroup writes as it starts, yielding its core between polls (sched_yield: no busy
        // spin), at most 20 ms.  Until round 4 it first slept on an event recorded before each classify
        // launch; that marker cost the stream a 6-us gap per batch (PPE_FLOW_EVENT=1 restores it, for A/B).
        if (t.use_event) HIPCHK(c, hipEventSynchronize(t.pre_launch));
        const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
        while (t.snap_used + 1u < t.batches && std::chrono::steady_clock::now() < until) {
            if (t.use_event) __builtin_ia32_pause();
            else sched_yield();
            flow_apply_snapshot(t);
        }
    }
    rc = flow_maybe_rehash(c);
    if (rc != PPE_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const ppe_flowdev d = flow_dev(t, t.cur);
    if (t.use_event) HIPCHK(c, hipEventRecord(t.pre_launch, s));
    // (the same for both launch shapes: the host's bounds, the snapshot ring and the parity follow the batch)
    const bool may_overflow = t.live_ub + in->n > t.capacity;
    // (with the detector, a claim whose claimers were all dropped leaves a tombstone too)
    const bool may_tomb = may_overflow || fps == PPE_FPS_KERNEL;
    // a small batch: classify and finalize in one launch of one workgroup, the found flows' updates by the direct
    // atomics (no owner buckets, no update workgroups).  Not with monitors flow-attached (their syncount count lives
    // in the post kernel), not while the post-launch failure hook is armed
    const bool small = fps != PPE_FPS_KERNEL &&
                       ppe_pick_flow_small(in->n, t.small_allowed && __atomic_load_n(&g_fail_post, __ATOMIC_RELAXED) == 0u,
                                           c->atk_flow != nullptr) != 0u;
    // the same launch shape with the monitors in it, for a chunk of the ports call only
    const bool small_atk = fps != PPE_FPS_KERNEL &&
                           ppe_pick_flow_small_attack(in->n, t.small_allowed && __atomic_load_n(&g_fail_post, __ATOMIC_RELAXED) == 0u,
                                                      c->atk_flow != nullptr, ports_call) != 0u;
    if (fst_ps) {
        // FlowHandlePacket with PortScan_Detect on its misses, then StreamTcp: one launch of one workgroup (kinds 7 / 8)
        rc = ps_reserve_keys(pt, in->n);  // (may synchronise and rebuild the detector's table; nothing enqueued yet)
        if (rc != PPE_OK) return rc;
        ppe_ps_kargs pa;
        ps_table_args(*pt, pa);
        pa.ts = in->ts;
        pa.ts_default = cfg ? cfg->now_seconds : 0u;
        pa.n = in->n;
        pa.now_cycles = pt->now_cycles;
        pa.now_seconds = pt->now_seconds;
        pa.freq = pt->cfg.exception_freq;
        pa.hold_seconds = pt->cfg.hold_seconds;
        pa.action = pt->cfg.action;
        ppe_flowdev ds = d;
        ds.upd_wgs = 0;
        const ppe_flow_small_tail tail = {in->len,      out->verdict, out->acl_hit, out->fw_idx, out->drop_idx,
                                          out->tile_cnt, out->part8,  0u,           0u};
        const ppe_flow_st_args sa = {t.arr[t.cur].sess, c->d_stc, t.tuple_scr};
        rc = launch(c, in, out, 1, cfg, s, 0, 0, &ds, nullptr, 0, &tail, &pa, false, false, atk_pb, true, &sa, fst_atk);
        if (rc != PPE_OK) return rc;  // (nothing ran: both tables are as they were)
    } else if (fst == PPE_FST_KERNEL) {
        // FlowHandlePacket, then StreamTcp for the TCP packets that have a flow: one launch of one workgroup
        ppe_flowdev ds = d;
        ds.upd_wgs = 0;
        const ppe_flow_small_tail tail = {in->len,      out->verdict, out->acl_hit, out->fw_idx, out->drop_idx,
                                          out->tile_cnt, out->part8,  may_overflow ? 1u : 0u, 0u};
        const ppe_flow_st_args sa = {t.arr[t.cur].sess, c->d_stc, t.tuple_scr};
        rc = launch(c, in, out, 1, cfg, s, 0, 0, &ds, nullptr, 0, &tail, nullptr, false, false, atk_pb, true, &sa, fst_atk);
        if (rc != PPE_OK) return rc;  // (nothing ran: the table is as it was)
    } else if (fps == PPE_FPS_KERNEL) {
        rc = ps_reserve_keys(pt, in->n);  // (may synchronise and rebuild the detector's table; nothing enqueued yet)
        if (rc != PPE_OK) return rc;
        ppe_ps_kargs pa;
        ps_table_args(*pt, pa);
        pa.ts = in->ts;
        pa.ts_default = cfg ? cfg->now_seconds : 0u;
        pa.n = in->n;
        pa.now_cycles = pt->now_cycles;
        pa.now_seconds = pt->now_seconds;
        pa.freq = pt->cfg.exception_freq;
        pa.hold_seconds = pt->cfg.hold_seconds;
        pa.action = pt->cfg.action;
        ppe_flowdev ds = d;
        ds.upd_wgs = 0;
        const ppe_flow_small_tail tail = {in->len,      out->verdict, out->acl_hit, out->fw_idx, out->drop_idx,
                                          out->tile_cnt, out->part8,  0u,           0u};
        rc = launch(c, in, out, 1, cfg, s, 0, 0, &ds, nullptr, 0, &tail, &pa, fpc == PPE_FPC_KERNEL, false, atk_pb, true);
        if (rc != PPE_OK) return rc;  // (nothing ran: both tables are as they were)
    } else if (small || small_atk) {
        ppe_flowdev ds = d;
        ds.upd_wgs = 0;
        const ppe_flow_small_tail tail = {in->len,      out->verdict, out->acl_hit, out->fw_idx, out->drop_idx,
                                          out->tile_cnt, out->part8,  may_overflow ? 1u : 0u, 0u};
        rc = launch(c, in, out, 1, cfg, s, 0, 0, &ds, nullptr, 0, &tail, nullptr, false, small_atk, atk_pb, true);
        if (rc != PPE_OK) return rc;  // (nothing ran: the table is as it was)
    } else {
        // 1. decode, hash, FlowFind; found flows are forwarded and their updates logged to the owners' buckets, the
        // rest get syn_check + ACL (would-be creators claim their slots)
        uint32_t cgrid = 0;
        rc = launch(c, in, out, 1, cfg, s, 0, 0, &d, &cgrid, 0, nullptr, nullptr, false, false, atk_pb, true);
        if (rc != PPE_OK) return rc;
        ppe_flow_kargs k;
        std::memset(&k, 0, sizeof k);
        k.f = d;
        k.f.upd_grid = cgrid;
        k.len = in->len;
        k.verdict = out->verdict;
        k.hit = out->acl_hit;
        k.fw_idx = out->fw_idx;
        k.drop_idx = out->drop_idx;
        k.tile_cnt = out->tile_cnt;
        k.part8 = out->part8;
        k.n = in->n;
        k.unsup_fw = cfg ? cfg->unsupport_proto_action : 0u;
        k.now = cfg ? cfg->now_seconds : 0u;
        k.nslots = t.nslots;
        k.cslots = c->d_cslots;
        if (ppe_pick_attack_flow(1, c->atk_flow != nullptr)) {  // syncount_accum: the flows this batch's SYNs create
            k.atk_slots = c->atk_flow->d_slots;
            k.atk_pb = atk_pb;
        }
        // 2. the post-classify launch: finalize (grid-stride over the miss-tile list, usually short: at most one
        // workgroup per CU) and, beside it, the found flows' counters and last-seen times, one workgroup per owner
        // (disjoint from the slots finalize touches).  When the host's bound says the pool may overflow, finalize checks
        // the exact counts and, on an overflow, marks the creators and has its workgroup 0 revoke those past the pool's
        // room first.
        // (fg <= n_cu <= max_grid: the finalize workgroups' indices stay inside the monitors' max_grid count slots)
        const uint32_t fg = std::min(std::min(flow_grid(c, (in->n + 63u) / 64u, PPE_FLOW_POST_BLOCK / 64u), c->n_cu),
                                     t.fin_cap ? t.fin_cap : c->n_cu);
        k.revoke = may_overflow ? 1u : 0u;
        k.fin_wgs = fg;
        {
            const int e = take_fail_post() ? (int)hipErrorLaunchFailure
                                           : ppe_launch_flow(PPE_FLOW_K_POST, &k, fg + (t.upd_wgs ? t.upd_owners : 0u), (void *)s);
            if (e != 0) {
                t.broken = true;  // the classify launch above claimed slots that nothing will finalize
                return fail(c, PPE_EIO, "flow post-classify launch failed: %s", hipGetErrorString((hipError_t)e));
            }
        }
    }
    t.last_kind = fst_ps ? (fst_atk ? 8u : 7u) : fst_atk ? 6u : fst == PPE_FST_KERNEL ? 5u : fpc == PPE_FPC_KERNEL ? 3u : fps == PPE_FPS_KERNEL ? 2u : small_atk ? 4u
                  : small ? 1u : 0u;
    t.last_launches = (fst == PPE_FST_KERNEL || fps == PPE_FPS_KERNEL || small || small_atk) ? 1u : 2u;
    t.cum_n[t.batches % FlowTable::kSnapRing] = t.tot_n;
    t.cum_rev[t.batches % FlowTable::kSnapRing] = t.tot_rev;
    t.tot_n += in->n;
    if (may_tomb) t.tot_rev += in->n;
    ++t.batches;
    t.live_ub = std::min<uint64_t>(t.live_ub + in->n, t.capacity);
    if (may_tomb) t.tomb_ub += in->n;  // revoked claims leave tombstones
    return PPE_OK;
}

int ppe_classify_flow(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                      void *stream) {
    // the monitors' port bytes: entry 0 of ppe_attack_ports' sticky table
    const uint8_t *pb = (c && c->atk_flow && !c->atk_flow->h_ports.empty()) ? c->atk_flow->h_ports[0] : nullptr;
    return classify_flow_run(c, in, out, cfg, stream, pb, false);
}

// ppe_classify_flow for a host-resident batch: consecutive flow batches of at most `chunk` packets, every copy and
// launch on c->host_cs in chunk order.  The flow path is exactly sequential, so the chunk size changes nothing.
// ports_call (ppe_classify_flow_host_ports): monitors may be flow-attached; every chunk's slice of the host array
// `ports` (NULL: port 0) is what they read, not the sticky table.  Between two ticks a monitor's verdict depends only on
// the packet and the interval's starting state (§5.8), and no tick lies inside a call, so the chunks compose to one
// core's run of the whole batch.
static int classify_flow_host_run(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                                  uint32_t chunk, const uint8_t *ports, bool ports_call) {
    if (!c || !out) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    if (!out->verdict) return fail(c, PPE_EINVAL, "ppe_classify_flow_host needs the verdict output");
    // the post kernel has no index base for a chunk's lists
    if (out->fw_idx || out->drop_idx || out->tile_cnt || out->part8 || out->packed)
        return fail(c, PPE_EINVAL, "ppe_classify_flow_host takes the per-packet outputs only (no lists, no packed)");
    // ppe_classify_flow's refusals, before anything is touched
    // (sessions attached and tracking on: every chunk is a session batch, with the monitors in it or without)
    const uint32_t fstm = flow_stream_pick(c, 1u);
    const uint32_t fst = (fst_has_atk(fstm) || fst_has_ps(fstm)) ? (uint32_t)PPE_FST_KERNEL : fstm;
    if (c->stcp.track && fst == PPE_FST_PLAIN)
        return fail(c, PPE_ENOTSUP, "ppe_classify_flow_host with stream tracking on is not supported");
    if (fst == PPE_FST_REFUSE) return flow_stream_refuse(c);
    if (c->ps) return fail(c, PPE_ENOTSUP, "ppe_classify_flow_host with a port-scan table attached is not supported");
    if (c->atk) return fail(c, PPE_ENOTSUP, "ppe_classify_flow_host with attack monitors attached is not supported");
    // the monitors' per-batch port array does not map onto chunks (as ppe_classify_host_ordered)
    if (c->atk_flow && !ports_call)
        return fail(c, PPE_ENOTSUP, "ppe_classify_flow_host with attack monitors flow-attached is not supported");
    if (!c->atk_flow) ports = nullptr;  // nothing reads them: exactly ppe_classify_flow_host
    // both flow-attached, the detector on and ppe_flow_combine off: ppe_classify_flow's refusal, before anything is touched
    if (ppe_pick_flow_combined(ppe_pick_flow_portscan(1u, c->ps_flow != nullptr, c->ps_flow ? c->ps_flow->cfg.able : 0u),
                               c->atk_flow != nullptr, c->flow_combine) == PPE_FPC_REFUSE)
        return fail(c, PPE_ENOTSUP, "ppe_classify_flow with a port-scan table and attack monitors both flow-attached "
                                    "is not supported");
    int rc = check_batch(c, in, cfg);
    if (rc != PPE_OK || in->n == 0) return rc;
    // the detector on (a table flow-attached, portscan_able 1): chunks of at most PPE_FLOW_PS_MAX packets, each one launch
    const bool fps = ppe_pick_flow_portscan(1u, c->ps_flow != nullptr, c->ps_flow ? c->ps_flow->cfg.able : 0u) != PPE_FPS_PLAIN;
    // session batches: chunks of at most PPE_FLOW_ST_MAX packets, each one launch
    if (fst == PPE_FST_KERNEL && in->stride < PPE_FLOW_STREAM_MIN_STRIDE)
        return fail(c, PPE_EINVAL, "ppe_classify_flow_host with TCP sessions needs a header stride of at least %u B",
                    PPE_FLOW_STREAM_MIN_STRIDE);
    // (both: chunks of at most the smaller of the two, inside both tables' max_batch)
    const uint32_t bmax = fst_has_ps(fstm) ? std::min(std::min(c->flow->max_batch, c->ps_flow->cfg.max_batch),
                                                      std::min(PPE_FLOW_ST_MAX, PPE_FLOW_PS_MAX))
                          : fst == PPE_FST_KERNEL ? std::min(c->flow->max_batch, PPE_FLOW_ST_MAX)
                          : fps ? std::min(c->flow->max_batch, std::min(c->ps_flow->cfg.max_batch, PPE_FLOW_PS_MAX))
                                : c->flow->max_batch;
    const uint32_t cmax = bmax & ~63u;
    if (cmax < 64u)
        return fail(c, PPE_EINVAL, "ppe_classify_flow_host: the %s table's max_batch is below one tile",
                    (c->flow->max_batch & ~63u) < 64u ? "flow" : "port-scan");
    HIPCHK(c, use_device(c));
    if (!c->host_cs) HIPCHK(c, hipStreamCreateWithFlags(&c->host_cs, hipStreamNonBlocking));
    const hipStream_t s = c->host_cs;
    // the monitors' set / tick kernels ran on the stream of the latest classify call (the legacy default stream before
    // the first); the internal stream does not wait for another one, so what was enqueued there completes first
    if (c->atk_flow && c->atk_flow->stream != s) HIPCHK(c, hipStreamSynchronize(c->atk_flow->stream));
    // Zero-copy: every buffer pinned and device-mapped, one batch: the kernels read and write the host buffers
    if (env_int("PPE_HOST_ZEROCOPY", 1) && in->n <= bmax) {
        ppe_batch_t b = *in;
        ppe_result_t r = *out;
        bool ok = (b.hdr = (const uint8_t *)mapped_host(in->hdr)) && (b.len = (const uint32_t *)mapped_host(in->len));
        if (in->ts) ok = ok && (b.ts = (const uint64_t *)mapped_host(in->ts));
        uint32_t **outs[] = {&r.verdict, &r.flow_hash, (uint32_t **)&r.acl_hit, &r.tuple};
        for (uint32_t **o : outs)
            if (ok && *o) ok = (*o = (uint32_t *)mapped_host(*o)) != nullptr;
        // (the ports call: only with no port array, or one that is itself pinned and device-mapped)
        const uint8_t *dp = ports ? (const uint8_t *)mapped_host(ports) : nullptr;
        if (ports && !dp) ok = false;
        if (ok) {
            rc = ports_call ? classify_flow_run(c, &b, &r, cfg, (void *)s, dp, true)
                            : ppe_classify_flow(c, &b, &r, cfg, (void *)s);
            HIPCHK(c, hipStreamSynchronize(s));
            return rc;
        }
    }
    if (chunk == 0) chunk = 1u << 18;
    chunk = (chunk + 63u) & ~63u;
    chunk = std::min(std::min(chunk, cmax), (in->n + 63u) & ~63u);
    rc = host_stages_reserve(c, chunk, in->stride);
    if (rc != PPE_OK) return rc;
    const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
    hipError_t he = hipSuccess;
    for (uint32_t base = 0, i = 0; base < in->n && rc == PPE_OK && he == hipSuccess; base += chunk, ++i) {
        HostStage &h = c->hs[i % kHostStreams];  // (one stream: a slot's reuse follows its last download)
        const uint32_t m = std::min(chunk, in->n - base);
        he = hipMemcpyAsync(h.hdr, in->hdr + (size_t)base * in->stride, (size_t)m * in->stride, h2d, s);
        if (he == hipSuccess) he = hipMemcpyAsync(h.len, in->len + base, (size_t)m * 4, h2d, s);
        if (he == hipSuccess && in->ts) he = hipMemcpyAsync(h.ts, in->ts + base, (size_t)m * 8, h2d, s);
        if (he == hipSuccess && ports) he = hipMemcpyAsync(h.ports, ports + base, (size_t)m, h2d, s);
        if (he != hipSuccess) break;
        ppe_batch_t b = {h.hdr, h.len, in->ts ? h.ts : nullptr, m, in->stride};
        ppe_result_t r;
        std::memset(&r, 0, sizeof r);
        r.verdict = h.verdict;
        r.flow_hash = out->flow_hash ? h.fhash : nullptr;
        r.acl_hit = out->acl_hit ? h.hit : nullptr;
        r.tuple = out->tuple ? h.tuple : nullptr;
        rc = ports_call ? classify_flow_run(c, &b, &r, cfg, (void *)s, ports ? h.ports : nullptr, true)
                        : ppe_classify_flow(c, &b, &r, cfg, (void *)s);
        if (rc != PPE_OK) break;
        he = hipMemcpyAsync(out->verdict + base, h.verdict, (size_t)m * 4, d2h, s);
        if (he == hipSuccess && out->flow_hash) he = hipMemcpyAsync(out->flow_hash + base, h.fhash, (size_t)m * 4, d2h, s);
        if (he == hipSuccess && out->acl_hit) he = hipMemcpyAsync(out->acl_hit + base, h.hit, (size_t)m * 4, d2h, s);
        if (he == hipSuccess && out->tuple)
            he = hipMemcpyAsync(out->tuple + (size_t)base * 4, h.tuple, (size_t)m * 16, d2h, s);
    }
    // (also after a failure: no copy into the caller's buffers is left in flight)
    const hipError_t se = hipStreamSynchronize(s);
    if (rc != PPE_OK) return rc;
    HIPCHK(c, he);
    HIPCHK(c, se);
    return PPE_OK;
}

int ppe_classify_flow_host(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                           uint32_t chunk) {
    return classify_flow_host_run(c, in, out, cfg, chunk, nullptr, false);
}

int ppe_classify_flow_host_ports(ppe_ctx_t *c, const ppe_batch_t *in, const ppe_result_t *out, const ppe_cfg_t *cfg,
                                 uint32_t chunk, const uint8_t *ports) {
    return classify_flow_host_run(c, in, out, cfg, chunk, ports, true);
}

int ppe_flow_launch_info(ppe_ctx_t *c, uint32_t *kind, uint32_t *launches) {
    if (!c || !kind || !launches) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    *kind = c->flow->last_kind;
    *launches = c->flow->last_launches;
    return PPE_OK;
}

int ppe_flow_portscan_rounds(ppe_ctx_t *c, uint32_t *rounds) {
    if (!c || !rounds) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    HIPCHK(c, use_device(c));
    HIPCHK(c, hipDeviceSynchronize());
    unsigned long long w = 0;
    HIPCHK(c, hipMemcpy(&w, c->flow->ctl + PPE_FCTL_PS_ROUNDS, 8, hipMemcpyDeviceToHost));
    *rounds = (uint32_t)w;
    return PPE_OK;
}

int ppe_flow_age(ppe_ctx_t *c, uint64_t now_seconds, uint64_t timeout_seconds, uint64_t *deleted) {
    if (!c) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    HIPCHK(c, use_device(c));
    FlowTable &t = *c->flow;
    unsigned long long before[PPE_FCTL_WORDS], after[PPE_FCTL_WORDS];
    int rc = flow_sync_counts(c, before);
    if (rc != PPE_OK) return rc;
    ppe_flow_kargs k;
    std::memset(&k, 0, sizeof k);
    k.f = flow_dev(t, t.cur);
    k.now = now_seconds;
    k.timeout = timeout_seconds;
    k.nslots = t.nslots;
    // monitors and sessions together (ppe_flow_stream_monitors): StreamTcp_Flow_ResRelease's syncount_accum decrements
    // for the flows the age kernel is about to delete, by a pass ahead of it on the same stream
    if (c->flow_st_monitors == 1u && t.stream_on && t.arr[t.cur].sess && c->atk_flow) {
        ppe_flow_st_age_kargs ra;
        std::memset(&ra, 0, sizeof ra);
        ra.keys = k.f.keys;
        ra.packed = k.f.packed;
        ra.sess = t.arr[t.cur].sess;
        ra.atk_slots = c->atk_flow->d_slots;
        ra.now = now_seconds;
        ra.timeout = timeout_seconds;
        ra.nslots = t.nslots;
        rc = ppe_launch_flow_stream_age_release(&ra, flow_grid(c, t.nslots, 256u), nullptr);
        if (rc != 0) return fail(c, PPE_EIO, "flow age launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    rc = ppe_launch_flow(PPE_FLOW_K_AGE, &k, flow_grid(c, t.nslots, 256u), nullptr);
    if (rc != 0) return fail(c, PPE_EIO, "flow age launch failed: %s", hipGetErrorString((hipError_t)rc));
    rc = flow_sync_counts(c, after);
    if (rc != PPE_OK) return rc;
    if (deleted) *deleted = after[PPE_FCTL_DEL_FLOW] - before[PPE_FCTL_DEL_FLOW];
    return flow_maybe_rehash(c);
}

int ppe_flow_info(ppe_ctx_t *c, ppe_flow_info_t *info) {
    if (!c || !info) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    HIPCHK(c, use_device(c));
    unsigned long long ctl[PPE_FCTL_WORDS];
    const int rc = flow_sync_counts(c, ctl);
    if (rc != PPE_OK) return rc;
    std::memset(info, 0, sizeof *info);
    const FlowTable &t = *c->flow;
    info->live = ctl[PPE_FCTL_LIVE];
    info->new_flow = ctl[PPE_FCTL_NEW_FLOW];
    info->del_flow = ctl[PPE_FCTL_DEL_FLOW];
    info->capacity = t.capacity;
    info->max_batch = t.max_batch;
    info->slots = t.nslots;
    info->tombstones = (uint32_t)ctl[PPE_FCTL_TOMBS];
    info->rehashes = t.rehashes;
    return PPE_OK;
}

int ppe_flow_clear_stat(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    HIPCHK(c, use_device(c));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemset(c->flow->ctl + PPE_FCTL_NEW_FLOW, 0, 16u));  // new_flow, del_flow
    return PPE_OK;
}

int ppe_flow_dump(ppe_ctx_t *c, ppe_flow_entry_t *entries, uint32_t max, uint32_t *n) {
    if (!c || !n) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    HIPCHK(c, use_device(c));
    HIPCHK(c, hipDeviceSynchronize());
    const FlowTable &t = *c->flow;
    const FlowArrays &a = t.arr[t.cur];
    constexpr uint32_t W = PPE_FLOW_SLOT_WORDS;
    std::vector<uint32_t> keys((size_t)t.nslots * W);
    HIPCHK(c, hipMemcpy(keys.data(), a.keys, keys.size() * 4u, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> stats, recs;
    if (entries && max) {
        stats.resize((size_t)t.nslots * 4u);
        HIPCHK(c, hipMemcpy(stats.data(), a.stats, stats.size() * 8u, hipMemcpyDeviceToHost));
        recs.resize((size_t)t.nslots * PPE_FLOW_REC_WORDS);
        HIPCHK(c, hipMemcpy(recs.data(), a.recs, recs.size() * 8u, hipMemcpyDeviceToHost));
    }
    uint32_t k = 0;
    for (uint32_t s = 0; s < t.nslots; ++s) {
        const uint32_t *kw = &keys[(size_t)W * s], st = kw[3];
        if ((st & (PPE_FS_PEND | 0xffu)) != PPE_FS_LIVE(0u)) continue;
        if (entries && k < max) {
            ppe_flow_entry_t &e = entries[k];
            std::memset(&e, 0, sizeof e);
            e.sip = kw[0];
            e.dip = kw[1];
            e.sport = (uint16_t)(kw[2] & 0xffffu);
            e.dport = (uint16_t)(kw[2] >> 16);
            e.protocol = (uint8_t)(st >> 8);
            e.slot = s;
            const unsigned long long *pr = &recs[(size_t)PPE_FLOW_REC_WORDS * s];  // packed counters, last-seen
            const unsigned long long bmask = (1ull << PPE_PK_SHIFT) - 1u, p0 = pr[0], p1 = pr[1];
            e.pktcnts2d = stats[4u * s] + (p0 >> PPE_PK_SHIFT);
            e.bytecnts2d = stats[4u * s + 1u] + (p0 & bmask);
            e.pktcntd2s = stats[4u * s + 2u] + (p1 >> PPE_PK_SHIFT);
            e.bytecntd2s = stats[4u * s + 3u] + (p1 & bmask);
            e.last_seen = pr[PPE_FLOW_REC_LAST];
        }
        ++k;
    }
    *n = k;
    return PPE_OK;
}

// ---- StreamTcp's session machine behind the flow table (csrc/ppe_kernels_flow_stream.hip) ----
uint32_t ppe_flow_stream_max(void) { return PPE_FLOW_ST_MAX; }

int ppe_flow_stream_attach(ppe_ctx_t *c, uint32_t on) {
    if (!c) return PPE_EINVAL;
    if (on > 1u) return fail(c, PPE_EINVAL, "ppe_flow_stream_attach: on must be 0/1");
    if (const int u = flow_usable(c)) return u;
    FlowTable &t = *c->flow;
    if (!on) {  // (the records stay allocated until ppe_flow_destroy; the next attach zeroes them)
        t.stream_on = false;
        return PPE_OK;
    }
    HIPCHK(c, use_device(c));
    HIPCHK(c, hipDeviceSynchronize());
    FlowArrays &a = t.arr[t.cur];
    if (!a.sess && hipMalloc(&a.sess, (size_t)t.nslots * 4u * PPE_FLOW_SESS_WORDS) != hipSuccess)
        return fail(c, PPE_ENOMEM, "ppe_flow_stream_attach: out of device memory (%u session records)", t.nslots);
    if (!t.tuple_scr && hipMalloc(&t.tuple_scr, (size_t)PPE_FLOW_ST_MAX * 16u) != hipSuccess)
        return fail(c, PPE_ENOMEM, "ppe_flow_stream_attach: out of device memory");
    if (!c->d_stc) {
        if (hipMalloc(&c->d_stc, PPE_STC_WORDS * 8u) != hipSuccess)
            return fail(c, PPE_ENOMEM, "ppe_flow_stream_attach: out of device memory");
        HIPCHK(c, hipMemset(c->d_stc, 0, PPE_STC_WORDS * 8u));
    }
    // attaching zeroes every record: flows alive now have no session (ssn == NULL in the reference)
    HIPCHK(c, hipMemset(a.sess, 0, (size_t)t.nslots * 4u * PPE_FLOW_SESS_WORDS));
    HIPCHK(c, hipDeviceSynchronize());
    t.stream_on = true;
    return PPE_OK;
}

// monitors flow-attached and sessions attached on one batch (csrc/ppe_kernels_flow_stream_attack.hip).
// Like ppe_flow_combine it is the context's: ppe_flow_destroy leaves it
int ppe_flow_stream_monitors(ppe_ctx_t *c, uint32_t on) {
    if (!c) return PPE_EINVAL;
    if (on > 1u) return fail(c, PPE_EINVAL, "ppe_flow_stream_monitors: on must be 0 or 1");
    c->flow_st_monitors = on;
    return PPE_OK;
}

// a port-scan table flow-attached (able 1) and sessions attached on one batch (csrc/ppe_kernels_flow_portscan_stream.hip,
// csrc/ppe_kernels_flow_portscan_attack_stream.hip).  The context's, like ppe_flow_combine and
// ppe_flow_stream_monitors: ppe_flow_destroy leaves it
int ppe_flow_stream_portscan(ppe_ctx_t *c, uint32_t on) {
    if (!c) return PPE_EINVAL;
    if (on > 1u) return fail(c, PPE_EINVAL, "ppe_flow_stream_portscan: on must be 0 or 1");
    c->flow_st_portscan = on;
    return PPE_OK;
}

int ppe_flow_stream_dump(ppe_ctx_t *c, ppe_flow_stream_entry_t *entries, uint32_t max, uint32_t *n) {
    if (!c || !n) return PPE_EINVAL;
    if (const int u = flow_usable(c)) return u;
    const FlowTable &t = *c->flow;
    const FlowArrays &a = t.arr[t.cur];
    if (!t.stream_on || !a.sess) return fail(c, PPE_EINVAL, "ppe_flow_stream_dump: no sessions attached (ppe_flow_stream_attach)");
    HIPCHK(c, use_device(c));
    HIPCHK(c, hipDeviceSynchronize());
    constexpr uint32_t W = PPE_FLOW_SLOT_WORDS, S = PPE_FLOW_SESS_WORDS;
    std::vector<uint32_t> keys((size_t)t.nslots * W), sess;
    HIPCHK(c, hipMemcpy(keys.data(), a.keys, keys.size() * 4u, hipMemcpyDeviceToHost));
    if (entries && max) {
        sess.resize((size_t)t.nslots * S);
        HIPCHK(c, hipMemcpy(sess.data(), a.sess, sess.size() * 4u, hipMemcpyDeviceToHost));
    }
    uint32_t k = 0;
    for (uint32_t s = 0; s < t.nslots; ++s) {
        const uint32_t *kw = &keys[(size_t)W * s];
        if (kw[3] != PPE_FS_LIVE(6u)) continue;
        if (entries && k < max) {
            ppe_flow_stream_entry_t &e = entries[k];
            std::memset(&e, 0, sizeof e);
            const uint32_t *w = &sess[(size_t)S * s];
            e.sip = kw[0];
            e.dip = kw[1];
            e.sport = (uint16_t)(kw[2] & 0xffffu);
            e.dport = (uint16_t)(kw[2] >> 16);
            e.slot = s;
            e.state = (uint8_t)(w[0] & 0xffu);
            e.flags = (uint16_t)(w[0] >> 8);
            e.pad = (uint8_t)(w[13] & 3u);  // flow_item_t.input_port (0 unless created under ppe_flow_stream_monitors)
            ppe_stream_side_t *side[2] = {&e.client, &e.server};
            for (int i = 0; i < 2; ++i) {
                const uint32_t *q = w + 1 + 6 * i;
                side[i]->flags = (uint16_t)(q[0] & 0xffffu);
                side[i]->wscale = (uint8_t)(q[0] >> 16);
                side[i]->isn = q[1];
                side[i]->next_seq = q[2];
                side[i]->last_ack = q[3];
                side[i]->next_win = q[4];
                side[i]->window = q[5];
            }
        }
        ++k;
    }
    *n = k;
    return PPE_OK;
}

int ppe_stream_track_counters_read(ppe_ctx_t *c, ppe_stream_track_counters_t *out) {
    if (!c || !out) return PPE_EINVAL;
    static_assert(sizeof(ppe_stream_track_counters_t) == PPE_STC_WORDS * 8u, "the counter block");
    std::memset(out, 0, sizeof *out);
    if (!c->d_stc) return PPE_OK;  // (never attached: nothing counted)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out->c, c->d_stc, PPE_STC_WORDS * 8u, hipMemcpyDeviceToHost));
    return PPE_OK;
}

int ppe_stream_track_counters_clear(ppe_ctx_t *c) {
    if (!c) return PPE_EINVAL;
    if (!c->d_stc) return PPE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemset(c->d_stc, 0, PPE_STC_WORDS * 8u));
    return PPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Flow-hash steering across GPUs

int ppe_steer_partition(ppe_ctx_t *c, const uint32_t *verdict, const uint32_t *flow_hash, uint32_t n, uint32_t world,
                        uint32_t rank, uint32_t *perm, uint32_t *counts, void *stream) {
    if (!c) return PPE_EINVAL;
    if (world == 0 || world > PPE_STEER_MAX_WORLD || rank >= world)
        return fail(c, PPE_EINVAL, "world must be 1..%d and rank < world", PPE_STEER_MAX_WORLD);
    if (!counts || (n && (!verdict || !flow_hash || !perm))) return fail(c, PPE_EINVAL, "null argument");
    HIPCHK(c, use_device(c));
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)world * 4u, s));
        return PPE_OK;
    }
    const uint32_t tiles = (n + 63u) / 64u;
    const size_t need = (size_t)tiles * world * 4u;
    if (need > c->steer_cap) {
        HIPCHK(c, hipStreamSynchronize(s));  // the old buffer may be in use by queued work
        if (c->d_steer) HIPCHK(c, hipFree(c->d_steer));
        c->d_steer = nullptr;
        c->steer_cap = 0;
        HIPCHK(c, hipMalloc(&c->d_steer, need));
        c->steer_cap = need;
    }
    ppe_steer_kargs k;
    std::memset(&k, 0, sizeof k);
    k.verdict = verdict;
    k.flow_hash = flow_hash;
    k.n = n;
    k.world = world;
    k.rank = rank;
    k.tcount = c->d_steer;
    k.perm = perm;
    k.counts = counts;
    const uint32_t grid = std::max(1u, std::min((tiles + 3u) / 4u, c->n_cu * 8u));
    for (int phase = 0; phase < 3; ++phase) {
        const int e = ppe_launch_steer(phase, &k, grid, (void *)s);
        if (e != 0) return fail(c, PPE_EIO, "steer kernel %d: %s", phase, hipGetErrorString((hipError_t)e));
    }
    return PPE_OK;
}

static int rows(ppe_ctx_t *c, const void *src, uint32_t row_bytes, const uint32_t *perm, uint32_t n, void *dst,
                int scatter, void *stream) {
    if (!c) return PPE_EINVAL;
    if (row_bytes == 0 || row_bytes % 4u || row_bytes > 256u) return fail(c, PPE_EINVAL, "row_bytes: 4..256, x4");
    if (n == 0) return PPE_OK;
    if (!src || !dst || !perm) return fail(c, PPE_EINVAL, "null argument");
    HIPCHK(c, use_device(c));
    ppe_rows_kargs k = {(const uint8_t *)src, (uint8_t *)dst, perm, n, row_bytes, (uint32_t)scatter, 0u};
    const uint64_t words = (uint64_t)n * (row_bytes / 4u);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((words + 255u) / 256u, c->n_cu * 16u));
    const int e = ppe_launch_rows(&k, grid, stream);
    if (e != 0) return fail(c, PPE_EIO, "rows kernel: %s", hipGetErrorString((hipError_t)e));
    return PPE_OK;
}

int ppe_gather_rows(ppe_ctx_t *c, const void *src, uint32_t row_bytes, const uint32_t *perm, uint32_t n, void *dst,
                    void *stream) {
    return rows(c, src, row_bytes, perm, n, dst, 0, stream);
}

int ppe_scatter_rows(ppe_ctx_t *c, const void *src, uint32_t row_bytes, const uint32_t *perm, uint32_t n, void *dst,
                     void *stream) {
    return rows(c, src, row_bytes, perm, n, dst, 1, stream);
}

}  // extern "C"
