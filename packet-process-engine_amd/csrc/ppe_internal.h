/* ppe_internal.h — declarations shared between the engine (host) and the HIP kernel translation unit. */
#ifndef PPE_INTERNAL_H
#define PPE_INTERNAL_H

#include <stdint.h>

#include "ppe_hip.h"

/* One batch of a launch: inputs, outputs (NULL = skipped) and sizes, as in ppe_batch_t / ppe_result_t. */
struct ppe_bdesc {
    const uint8_t *hdr;
    const uint32_t *len;
    const uint64_t *ts;
    uint32_t *verdict;
    uint32_t *fhash;
    int32_t *hit;
    uint32_t *fw_idx;
    uint32_t *drop_idx;
    uint32_t *tile_cnt;
    uint32_t *tuple;
    uint32_t n;
    uint32_t stride;
    uint32_t idx_base;        /* added to the packet indices written to fw_idx / drop_idx */
    uint32_t flags;           /* PPE_BD_PART8: tile_cnt carries the compact partition list (ppe_result_t.part8);
                                 PPE_BD_PACKED: verdict carries the 8-B packed results (ppe_result_t.packed) */
};
#define PPE_BD_PART8 1u
#define PPE_BD_PACKED 2u
/* port-scan launches (ppe_kargs.psmask): flags >> PPE_BD_PSOFF_SHIFT = the word offset of the batch's drop mask (one
 * 64-bit word per tile) in ppe_kargs.psmask; the descriptor has no spare pointer and keeps its 96 bytes */
#define PPE_BD_PSOFF_SHIFT 2u

/* Device flow table (ppe_classify_flow; ppe_kernels.hip "flow table").  Open addressing over groups of
 * PPE_FLOW_GROUP slots, linear probing from group flow_hash & gmask; a key lies before the first EMPTY slot of its
 * probe sequence (slots never return to EMPTY: deletions leave TOMBs, reclaimed by a rehash).  The probe array holds
 * only the keys, 16 B per slot {sip, dip, sport | dport << 16, state}, so a probe group of 4 slots is one 64-B
 * segment: one HBM request per probe (round 5; until then a 64-B slot record with the counters inside, a 128-B line
 * per probe group of 2).  The counters live in a record array of their own, 32 B per slot: the packed counters of
 * both directions and the last-seen time (`packed`). */
#define PPE_FLOW_GROUP 4u       /* slots per probe group */
#define PPE_FLOW_SLOT_WORDS 4u  /* u32 words per slot key */
#define PPE_FLOW_REC_WORDS 4u   /* u64 stride of the counter records {s2d, d2s, last-seen, 0} */
#define PPE_FLOW_REC_LAST 2u    /* the counter record's last-seen time */
#define PPE_FS_EMPTY 0u
#define PPE_FS_TOMB 1u
#define PPE_FS_LIVE(proto) (2u | ((proto) << 8))  /* key words valid */
#define PPE_FS_PEND 0x80000000u                   /* | packet index: claimed by this batch, key = rec[index] */
#define PPE_FLOW_NONE 0xffffffffu
#define PPE_FLOW_REVOKED 0x80000000u              /* creator word: pool exhausted, the claim is withdrawn */
enum { PPE_FCTL_LIVE = 0, PPE_FCTL_NEW_FLOW, PPE_FCTL_DEL_FLOW, PPE_FCTL_BATCH_NEW, PPE_FCTL_TOMBS,
       PPE_FCTL_MISS0, PPE_FCTL_MISS1, /* tiles with pending packets, by batch parity */
       PPE_FCTL_REVOKED_SEQ,           /* finalize: workgroup 0's revoke published for batch seq + 1 */
       PPE_FCTL_ERR,                   /* finalize: waits for the revoke flag that gave up (results not exact) */
       PPE_FCTL_LIVE_AT_BATCH,         /* LIVE as the batch's classify launch started: every finalize workgroup takes
                                          its overflow decision from this word, which nothing changes during finalize
                                          (LIVE itself grows as finalize workgroups finish) */
       PPE_FCTL_BATCH_NEW1,            /* BATCH_NEW of odd batches: the creators (slots claimed) the classify launch
                                          counts, by batch parity; finalize reads its batch's and zeroes the next's */
       PPE_FCTL_ARRIVE,                /* finalize, overflow batches: workgroups done marking their tiles' creators */
       PPE_FCTL_PS_ROUNDS,             /* the last batch of the kernel with the port-scan detector inside: resolve rounds
                                          taken (debug count, ppe_flow_portscan_rounds) */
       PPE_FCTL_WORDS = 16 };
#define PPE_PK_SHIFT 40u                       /* packed counter: packets in bits 63:40, bytes in 39:0 */
#define PPE_PK_FOLD_PKTS (1ull << 23)          /* fold into `stats` once either field reaches half its range */
#define PPE_PK_FOLD_BYTES (1ull << 39)
/* Owner-computed FlowUpdate (flow_update_wg, ppe_flow_post_kernel): a found packet's counter update goes to a bucket of its slot's
 * owner (one of at most PPE_UPD_OWNERS slot ranges) in its classify workgroup's column, instead of a memory-side
 * atomic per packet; each owner's workgroup then sums its buckets in LDS and updates each touched slot once. */
#ifndef PPE_UPD_OWNERS
#define PPE_UPD_OWNERS 256u
#endif
#define PPE_UPD_CAP 16u        /* entries per (owner, classify workgroup) bucket; a full bucket: the direct atomic */
#ifndef PPE_UPD_HASH
#define PPE_UPD_HASH 4096u     /* LDS hash entries of an owner workgroup (slots it accumulates; more: direct atomics) */
#endif
#ifndef PPE_FLOW_POST_BLOCK
#define PPE_FLOW_POST_BLOCK 1024 /* workgroup size of the post-classify launch (finalize + update; 512: +1.4 µs per F1 batch) */
#endif
struct ppe_flowdev {
    uint32_t *keys;               /* nslots × {sip, dip, sport | dport << 16, state}: the key in the creating packet's
                                     orientation (the probe array)                                                     */
    unsigned long long *packed;   /* nslots × {s2d, d2s, last-seen, 0} (stride PPE_FLOW_REC_WORDS): packets << 40 |
                                     bytes per direction (FlowUpdate) and the last-seen time                          */
    unsigned long long *stats;    /* nslots × {pkts s2d, bytes s2d, pkts d2s, bytes d2s}: folded from `packed` before a
                                     field can overflow; a flow's counters = stats + the packed fields               */
    uint32_t *creator;            /* nslots: lowest index of the packets claiming the slot in this batch (| REVOKED)   */
    unsigned long long *ctl;      /* PPE_FCTL_* device counters                                                        */
    uint32_t *rec;                /* max_batch × {sip, dip, ports, proto | provisional status << 8} of pending packets */
    unsigned long long *tile_miss;  /* per tile: lanes whose flow was not found (pending resolution)                   */
    unsigned long long *tile_new;   /* per tile: lanes that create their flow                                          */
    uint32_t *rslot;              /* max_batch: the slot a pending packet's flow was claimed in, or PPE_FLOW_NONE       */
    uint32_t *miss_tiles;         /* tiles with pending packets (unordered), count in ctl[PPE_FCTL_MISS0 + parity]      */
    uint32_t parity;              /* batch sequence number & 1                                                         */
    unsigned long long fold_pkts, fold_bytes;  /* packed-counter fold thresholds (PPE_PK_FOLD_*; lowered by tests)   */
    unsigned long long *snap;     /* pinned host words {seq, live, tombstones}: written by the classify launch        */
    unsigned long long seq;       /* batches completed before this one                                                 */
    uint32_t gmask;               /* slot groups - 1                                                                   */
    uint32_t capacity;            /* flow pool size                                                                     */
    unsigned long long *upd;      /* [owner][upd_wgs][PPE_UPD_CAP]: slot | (wire length | dir << 31) << 32             */
    uint32_t *ucnt;               /* [upd_wgs][owner]: entries in each bucket (written by the classify launch)         */
    uint32_t upd_wgs;             /* classify workgroups with a bucket column (0: every found packet's atomic inline)  */
    uint32_t upd_osh;             /* owner of slot s = s >> upd_osh                                                      */
    uint32_t upd_owners;          /* owners (nslots >> upd_osh)                                                          */
    uint32_t upd_grid;            /* the update kernel: the batch's classify grid (bucket columns written)              */
    uint32_t upd_hmask;           /* the update kernel's LDS hash entries - 1 (PPE_UPD_HASH - 1; lowered by tests)       */
};

/* flow-table kernels after the classify kernel (one batch) */
struct ppe_flow_kargs {
    struct ppe_flowdev f;
    const uint32_t *len;          /* the batch's wire lengths (byte counters) */
    uint32_t *verdict;
    int32_t *hit;
    uint32_t *fw_idx, *drop_idx, *tile_cnt;
    uint8_t *part8;               /* compact partition list (ppe_result_t.part8) */
    uint32_t n;
    uint32_t unsup_fw;
    uint64_t now;
    uint64_t timeout;             /* aging */
    uint32_t nslots;
    uint32_t revoke;              /* finalize: the host's bound says the pool may overflow (check, rank, revoke) */
    uint32_t fin_wgs;             /* post-classify launch: workgroups [0, fin_wgs) finalize, the next upd_owners update */
    unsigned long long *cslots;   /* counter slots (one per workgroup) */
    union {
        struct ppe_flowdev dst;   /* rehash target */
        /* the post launch with attack monitors flow-attached (it has no rehash target: the same bytes, so the block
           keeps its size; atk_slots NULL: without): syncount_accum of the flows TCP SYN packets create
           (DP_Attack_SynCountMonitor in FlowAdd, flow.c:151-154) */
        struct {
            unsigned long long *atk_slots; /* [>= fin_wgs][PPE_ATK_SLOT_WORDS]: finalize workgroup b adds into slot b */
            const uint8_t *atk_pb;         /* the batch's port bytes or NULL (port 0) */
        };
    };
};

/* ---- one launch for small flow batches (csrc/ppe_kernels_flow_small.hip) ----
 * A flow batch of 1 <= n <= PPE_FLOW_SMALL_CUTOFF packets runs classify and finalize in one launch of one 1024-thread
 * workgroup instead of two launches sized for 1M-packet batches (ppe_pick_flow_small).  A multiple of 64, at least 64,
 * at most 2,048, and never above the largest size at which tools/ab_flow_small.py's measurement supports it. */
#define PPE_FLOW_SMALL_CUTOFF 512u
/* the same kernel with the flow-attached monitors in it (csrc/ppe_kernels_flow_small_attack.hip, launch kind 4;
 * ppe_pick_flow_small_attack): a multiple of 64, at most PPE_FLOW_SMALL_CUTOFF, and never above the
 * largest size at which tools/ab_flow_host_ports.py's measurement supports it on every workload (at 384 and above a batch
 * of nothing but new SYN flows measured 1.3-1.7 us slower than the two launches, beyond the A/A spread) */
#ifndef PPE_FLOW_SMALL_ATK_CUTOFF  /* (a measuring build may raise it: tools/ab_flow_host_ports.py) */
#define PPE_FLOW_SMALL_ATK_CUTOFF 256u
#endif
#define PPE_FLOW_SMALL_BLOCK 1024
/* what finalize needs beside the classify arguments (ppe_flow_kargs' fields of the same names; n, unsup_fw, now, the
 * counter slots and the table come from ppe_kargs) */
struct ppe_flow_small_tail {
    const uint32_t *len;
    uint32_t *verdict;
    int32_t *hit;
    uint32_t *fw_idx, *drop_idx, *tile_cnt;
    uint8_t *part8;
    uint32_t revoke;
    uint32_t pad;
};

/* ---- one launch for small fragment batches (csrc/ppe_defrag_small.hip) ----
 * A ppe_defrag batch of 1 <= n <= PPE_DEFRAG_SMALL_CUTOFF fragments runs its six phases in one launch of one
 * PPE_DEFRAG_SMALL_BLOCK-thread workgroup instead of six launches sized for 65,536-fragment batches
 * (ppe_pick_defrag_small).  At most the workgroup's threads (one fragment per thread in the per-fragment phases), and
 * never above the largest size at which tools/ab_defrag_small.py's measurement supports it. */
#define PPE_DEFRAG_SMALL_CUTOFF 4u
#define PPE_DEFRAG_SMALL_BLOCK 256

/* batches per launch whose descriptors travel in the kernel arguments (32 × 96 B); a launch over more batches reads
 * them from a device descriptor ring (ppe_kargs.ring) */
#define PPE_MAX_BATCH 32
/* most batches one ring launch takes */
#define PPE_MAX_RING 4096

/* Kernel launch parameters, passed by value. */
struct ppe_kargs {
    union {
    struct ppe_bdesc batch[PPE_MAX_BATCH];  /* [0, nbatch) when nbatch <= PPE_MAX_BATCH.  The grid's waves split into
                                               G = min(waves, nbatch, max_groups) batch groups that run concurrently:
                                               group g takes batches g, g + G, ... in turn (no barrier between them),
                                               its waves striding over each batch's tiles */
    /* Flow-table launches of a context with attack monitors flow-attached (ppe_flow_attack_attach; the FLOW + ATK
       kernels, csrc/ppe_kernels_attack_flow.hip).  There `flow` and the monitors' arguments below do meet; a
       flow-table launch is one batch, so its monitor arguments lie in the bytes of batch[1]: the argument block keeps
       its size and every offset (the implicit arguments behind it included), and no other kernel reads them
       (fatk_st NULL: the flow kernels without the monitors).  The batch's port bytes travel by value */
    struct {
        struct ppe_bdesc fatk_batch0;        /* = batch[0] */
        unsigned long long *fatk_st;         /* as atk_st */
        unsigned long long *fatk_slots;      /* as atk_slots; word 3 port + 2 (syncount_accum) is the post launch's */
        const uint8_t *fatk_pb;              /* the batch's port bytes (entry 0 of ppe_attack_ports' table) or NULL */
        uint64_t fatk_now;                   /* as atk_now */
        uint32_t fatk_hold;                  /* as atk_hold */
        uint32_t fatk_pad;
    };
    };
    const struct ppe_bdesc *ring;           /* non-NULL: the nbatch descriptors are ring[0, nbatch) in device memory
                                               (one persistent launch over a whole queue of batches, nbatch beyond
                                               PPE_MAX_BATCH); batch[0] then repeats ring[0] */
    uint32_t nbatch;
    uint32_t max_tiles;       /* largest batch's tile count */
    const uint32_t *img;      /* device classifier image (ppe_image.h) */
    uint32_t img_words;
    uint32_t unsup_fw;        /* 1: unsupported protocols are forwarded */
    uint32_t syn_check;
    uint32_t default_action;
    uint64_t now;
    uint32_t lds_words;       /* image words [0, lds_words) in LDS at its image base (single-tile walks; the leaf
                                 lists / rule records of every walk are read from LDS when inside this prefix)   */
    uint32_t stage_src, stage_words; /* the kernel stages image words [stage_src, + stage_words) at its LDS image base */
    uint32_t lds_blocks;      /* multi-tile walks: 2-level blocks [0, lds_blocks) are in LDS                        */
    uint32_t bsec_lds, blk_lds; /* LDS byte offsets (from the LDS image base) of the block section / of block 0     */
    uint32_t off_bsec, off_blocks, max_bdepth; /* image header words 15, 17, 18                                  */
    uint32_t off_crec, off_idtab; /* image header words 19, 20: compact leaf records / slot → index table (0 = none) */
    uint32_t crec_lds, idtab_lds; /* their LDS byte offsets from the LDS image base, ~0u = read from global memory   */
    uint32_t cut;             /* cut-list walks (image v8): cut header word 0 (sip bits | dip bits << 8 | ids16)     */
    uint32_t cut_slc, cut_gbase, cut_fp, cut_ent;  /* word offsets of the length slices / group bases / fingerprints /
                                                      entry lines in the image                                       */
    uint32_t cut_epl, cut_div;  /* entries per 128-B line, and the divisor magic (e / epl = umulhi(e, cut_div))      */
    uint32_t cut_idrel;         /* without PPE_CUT_LINES: the id array's byte offset from the entry lines             */
    uint32_t cut_gbase_lds, cut_fp_lds, cut_ent_lds;  /* their LDS byte offsets from the LDS image base (the slices
                                                         are at it; the entry lines: IMG_LDS only)                   */
    uint32_t max_groups;      /* most batch groups of waves (concurrently streamed batches)                          */
    uint32_t part_layout;     /* 1: every batch writes verdict + flow hash + ACL hit and one partition list (fw_idx ==
                                 drop_idx), no tile counts, no tuple: the kernel variant with those checks compiled out */
    uint32_t lds_iters;       /* IMG_SPLIT: walk levels (node reads) whose nodes are all in the staged BFS prefix      */
    uint32_t max_depth;       /* deepest leaf: the walk reads max_depth + 1 nodes                                     */
    uint32_t max_leaf;        /* longest leaf candidate list: uniform trip count of the leaf scan                     */
    uint32_t root_ks;         /* the root node's key slot << 8 (image header word PPE_IMG_W_ROOTKS)                    */
    uint32_t jump;            /* jump root descriptor (image header word PPE_IMG_W_JUMP), 0 = none                    */
    uint32_t off_nodes;       /* image word offset of the nodes (after the jump table)                                */
    uint32_t off_leaf, off_rules, off_resid; /* image section offsets (words), from the image header: kernel arguments
                                                (scalar registers, no load in the loop)                               */
    unsigned long long *cslots; /* [grid][PPE_CSLOT_WORDS] counter slots, one per workgroup */
    unsigned long long *sslots; /* [grid][PPE_SSLOT_WORDS] StreamTcp counter slots (enum ppe_stream_counter) */
    uint32_t stream;            /* StreamTcp first-packet verdict (ppe_stream_tcp_set): 0 = off, else PPE_STM_TRACK |
                                   PPE_STM_PICKUP (midstream or async_oneside: SYN|ACK passes); wave-uniform */
    /* the launch's completion, for the host's image / descriptor-ring reader bookkeeping (no event marker behind each
       launch): every workgroup, at its end, adds 1 to *done_cnt (a per-slot running count); the one that brings it to
       done_target writes done_seq to *done_host (pinned host memory).  done_cnt NULL: not tracked */
    unsigned long long *done_cnt, *done_host;
    unsigned long long done_target, done_seq;
    /* flow-table launches (ppe_classify_flow, one batch): `flow`.  Stateless launches of a context with a port-scan table
       attached and enabled (the PSC kernels, csrc/ppe_kernels_portscan.hip): `psmask`, the drop masks the pre-pass wrote,
       one 64-bit word per tile, batch b's at word ppe_bdesc.flags >> PPE_BD_PSOFF_SHIFT; NULL: the kernels without the
       detector.  The two never meet, so they share the bytes: the argument block keeps its size and every offset */
    /* Stateless launches of a context with attack monitors attached (the ATK kernels, csrc/ppe_kernels_attack*.hip):
       the fields behind psmask, in the same shared bytes (atk_st NULL: the kernels without the monitors) */
    union {
        struct ppe_flowdev flow;
        struct {
            const unsigned long long *psmask;
            unsigned long long *atk_st;          /* the object's device state (PPE_ATK_*), word 0 the decision word */
            unsigned long long *atk_slots;       /* [grid][PPE_ATK_SLOT_WORDS]: the workgroups' own count slots */
            const uint8_t *const *atk_ports;     /* device table: batch k's port bytes, or NULL; NULL: port 0 */
            uint64_t atk_now;                    /* ppe_attack_clock: OCT_TIME_SECONDS_SINCE1970 */
            uint32_t atk_hold;                   /* flood_hold_time */
            uint32_t atk_nports;                 /* entries of atk_ports */
            uint32_t atk_pbase;                  /* the call's batch index of this launch's batch 0 */
        };
    };
};

/* the one-launch flow kernel's own argument block: the classify arguments (ppe_kargs keeps its size and offsets), then
 * finalize's */
struct ppe_flow_small_kargs {
    struct ppe_kargs k;
    struct ppe_flow_small_tail t;
};

/* ---- attack monitors (csrc/ppe_attack.hip, the ATK classify kernels; dataplane/src/attack/dp_attack.c) ----
 * Counts: every classify workgroup adds its per-port accumulator counts and drop totals into a slot of its own
 * (PPE_ATK_SLOT_WORDS u64: [3 port + class] udp / syn / syncount accum, [12 + t] the drop totals), as the packet
 * counters do (cslots): no word is shared between workgroups.  The tick kernel folds the slots into the state and
 * zeroes them; ppe_attack_info adds what they hold.
 * Device state: u64 words.  [PPE_ATK_WORD] the decision word: port p's six bits at 6 p; [PPE_ATK_TOTALS + 0..3] the
 * land / udp-flood / syn-flood / syncount drop totals; port p's words at PPE_ATK_PORT0 + PPE_ATK_PORT_STRIDE p. */
#define PPE_ATK_LAND 1u        /* pd.land == 1 && pd.drop_pack == 1 */
#define PPE_ATK_UDP_DROP 2u    /* td.flood_udp == 1 && td.drop_pack == 1 && (hold || udppps > udp_speed) */
#define PPE_ATK_UDP_ARM 4u     /* UDP_DROP and no hold: the first dropped packet sets the hold */
#define PPE_ATK_SYN_DROP 8u
#define PPE_ATK_SYN_ARM 16u
#define PPE_ATK_SYNCOUNT 32u   /* syncount > td.syn_count && td.drop_pack == 1 */
enum { PPE_ATK_WORD = 0, PPE_ATK_TOTALS = 4, PPE_ATK_PORT0 = 8, PPE_ATK_PORT_STRIDE = 16,
       /* a port's words: the ten attack_info fields, then the rule reduced to what the monitors read */
       PPE_ATK_UDPPPS = 0, PPE_ATK_UDP_ACCUM, PPE_ATK_SYNPPS, PPE_ATK_SYN_ACCUM, PPE_ATK_SYNCNT, PPE_ATK_SYNCNT_ACCUM,
       PPE_ATK_SYN_HOLD, PPE_ATK_SYN_HOLD_TIME, PPE_ATK_UDP_HOLD, PPE_ATK_UDP_HOLD_TIME,
       PPE_ATK_RULE_EN /* PPE_ATK_EN_* */, PPE_ATK_UDP_SPEED, PPE_ATK_SYN_SPEED, PPE_ATK_SYN_COUNT,
       PPE_ATK_WORDS = 8 + 16 * 4 };
#define PPE_ATK_EN_LAND 1u     /* pd.land == 1 && pd.drop_pack == 1 */
#define PPE_ATK_EN_UDP 2u      /* td.flood_udp == 1 && td.drop_pack == 1 */
#define PPE_ATK_EN_SYN 4u      /* td.flood_syn == 1 && td.drop_pack == 1 */
#define PPE_ATK_EN_DROP 8u     /* td.drop_pack == 1 */
/* the bins (status 29-31, unused, | port << 5) that hold a workgroup's per-port udp_accum / syn_accum /
 * syncount_accum counts until its flush */
#define PPE_ATK_BIN_UDP 29u
#define PPE_ATK_BIN_SYN 30u
#define PPE_ATK_BIN_SYNCNT 31u
/* Dec.flags bits that carry the packet's input port to finish() (above the StreamTcp bits 16-21) */
#define PPE_ATK_PORT_SHIFT 22u
/* and, until the count that follows decode(), the accumulator it counts in: 0 none, 1 udp_accum, 2 syn_accum */
#define PPE_ATK_CLS_SHIFT 24u
#define PPE_ATK_SLOT_WORDS 16u
#define PPE_ATK_CTL_BLOCK 1024
enum { PPE_ATK_K_SET = 0, PPE_ATK_K_TICK = 1, PPE_ATK_K_CLEAR = 2 };
struct ppe_atk_kargs {
    unsigned long long *st;
    unsigned long long *slots;                   /* [nslots][PPE_ATK_SLOT_WORDS] */
    uint32_t nslots, pad0;
    uint64_t now;                                /* tick */
    uint32_t rule[4][4];                         /* set: EN bits, udp_speed, syn_speed, syn_count per port */
    uint32_t op, pad;
};

/* ---- port-scan detector (csrc/ppe_portscan.hip; dataplane/src/attack/dp_portscan.c) ----
 * Table: open addressing, linear probing from hash(sip); keys[s] = 0 (empty) or 1 << 32 | sip, never removed between
 * rebuilds (aging and slot reclamation rebuild the table); recs[s] = PPE_PS_REC_WORDS u64:
 *   [0] last_cycle [1] cycle [2] portscan_hold_time [3] exception | last_exception << 32
 *   [4] last_dport | PPE_PS_LIVE | PPE_PS_SERIAL | firstinv << 32
 * A key without PPE_PS_LIVE holds no record (a source refused with NOMEM keeps its slot until the next rebuild).
 * firstinv (batch scratch) = max over the batch's packets of a record-less source of ~index: its first appearance. */
#define PPE_PS_REC_WORDS 5u
#define PPE_PS_LIVE 0x10000u
#define PPE_PS_SERIAL 0x20000u   /* batch scratch: the source's packets go through the wave walker */
#define PPE_PS_NOSLOT 0xffffffffu
enum { PPE_PS_OK = 0, PPE_PS_NOMEM = 1, PPE_PS_DETECTED = 2, PPE_PS_HOLD = 3, PPE_PS_INELIGIBLE = 0xff };
enum { PPE_PSC_LIVE = 0, PPE_PSC_NEW, PPE_PSC_DEL, PPE_PSC_OK, PPE_PSC_NOMEM, PPE_PSC_DETECTED, PPE_PSC_HOLD,
       PPE_PSC_DROP, PPE_PSC_OCC /* keys in use */, PPE_PSC_WORK /* batch: sources queued for the walker */,
       PPE_PSC_FREE /* batch: capacity - live as the batch started */, PPE_PSC_WORDS = 16 };
#define PPE_PS_SORT_BLOCK 2048u   /* keys one workgroup sorts in LDS */
struct ppe_ps_kargs {
    unsigned long long *keys, *recs, *ctl;
    uint32_t smask;               /* slots - 1 */
    uint32_t capacity;
    /* the batch */
    const uint8_t *hdr;
    const uint32_t *len;
    const uint64_t *ts;
    uint32_t n, stride, syn_check, npad;   /* npad: sort length, a power of two >= max(n, PPE_PS_SORT_BLOCK) */
    uint64_t ts_default;          /* cfg->now_seconds: mbuf->timestamp without batch.ts */
    uint64_t now_cycles, now_seconds, rate;
    uint32_t freq, hold_seconds, action, sort_k, sort_j, pad;
    /* batch scratch */
    uint32_t *slot_of;            /* [n] the packet's slot or PPE_PS_NOSLOT */
    uint32_t *dport;              /* [n] */
    uint64_t *pts;                /* [n] mbuf->timestamp */
    unsigned long long *skey;     /* [npad] slot << 32 | index of the packets with a record, ~0 the rest; sorted */
    uint8_t *res;                 /* [n] PPE_PS_* */
    unsigned long long *cmask;    /* [tiles] packets that are their new source's first appearance */
    uint32_t *cbase;              /* [tiles] their count, then its exclusive prefix */
    uint32_t *work;               /* [n] sorted positions of the walker's sources */
    unsigned long long *mask;     /* [tiles] out: the batch's drop mask */
    /* rebuild */
    unsigned long long *dkeys, *drecs;
    uint32_t dmask, age;
    /* attack monitors attached as well: a packet they drop never reaches PortScan_Detect (the find kernel evaluates
       the classify kernel's predicate from the same decision word); atk_st NULL: none */
    const unsigned long long *atk_st;
    const uint8_t *atk_ports;     /* the batch's port bytes or NULL */
};
enum { PPE_PS_K_FIND = 0, PPE_PS_K_CREATORS, PPE_PS_K_SCAN, PPE_PS_K_GRANT, PPE_PS_K_KEYS, PPE_PS_K_SORT_LDS,
       PPE_PS_K_SORT_MERGE_LDS, PPE_PS_K_SORT_GLOBAL, PPE_PS_K_HEADS, PPE_PS_K_MEMBERS, PPE_PS_K_WALK, PPE_PS_K_MASK,
       PPE_PS_K_REBUILD, PPE_PS_K_FUSED /* find .. mask in one launch of one workgroup, n <= PPE_PS_SORT_BLOCK */ };
/* largest batch the one-launch pre-pass takes (ppe_pick_portscan_prepass).  tools/ab_portscan_small.py measures it
 * against the staged launches at 1 .. 2,048 packets */
#define PPE_PS_FUSED_CUTOFF PPE_PS_SORT_BLOCK

/* ---- the flow-table kernel with the port-scan detector inside (csrc/ppe_kernels_flow_portscan.hip) ----
 * A flow batch of 1 <= n <= PPE_FLOW_PS_MAX packets of a context with a table flow-attached (ppe_flow_portscan_attach)
 * and enabled: classify, resolve and finalize in one launch of one PPE_FLOW_PS_BLOCK-thread workgroup, one packet per
 * thread.  One of 512 / 1,024 / 2,048; 2,048 needs two packets per thread and 80 KB of resolve state, more than the
 * 42 KB of LDS the classify phase leaves free in front of every image placement. */
#define PPE_FLOW_PS_MAX 1024u
#define PPE_FLOW_PS_BLOCK 1024
/* the arguments of the one-launch flow kernel, then the detector's: the table and the clock of ppe_ps_kargs (keys, recs,
 * ctl, smask, capacity, ts, ts_default, now_cycles, now_seconds, rate, freq, hold_seconds, action; nothing else is read) */
struct ppe_flow_ps_kargs {
    struct ppe_kargs k;
    struct ppe_flow_small_tail t;
    struct ppe_ps_kargs ps;
};

/* ---- the flow-table kernel with the TCP session machine behind it (csrc/ppe_kernels_flow_stream.hip) ----
 * A flow batch of 1 <= n <= PPE_FLOW_ST_MAX packets of a context with sessions attached (ppe_flow_stream_attach) and
 * tracking on: classify, finalize, the session walk and the final verdicts in one launch of one PPE_FLOW_ST_BLOCK-thread
 * workgroup, one packet per thread.  The larger of 512 and 1,024 whose LDS (24.3 KB of sort keys, packet words and
 * counters in front of every image placement) and registers fit (DESIGN.md §5.15 has the numbers). */
#define PPE_FLOW_ST_MAX 1024u
#define PPE_FLOW_ST_BLOCK 1024
#define PPE_FLOW_SESS_WORDS 16u   /* u32 words of a session record (csrc/ppe_stream_session_dev.h has the layout) */
#define PPE_STC_WORDS 64u         /* the counter block: struct tcpstream_track_stat's 58 fields, 6 spare words */
/* the arguments of the one-launch flow kernel (its list pointers NULL in k and t: nothing is compacted before the
 * sessions have spoken), then the lists, the session records of the table's current slot arrays, the counter block */
struct ppe_flow_st_kargs {
    struct ppe_kargs k;
    struct ppe_flow_small_tail t;
    uint32_t *fw_idx, *drop_idx, *tile_cnt;
    uint8_t *part8;
    uint32_t *sess;               /* nslots x PPE_FLOW_SESS_WORDS */
    unsigned long long *stc;      /* PPE_STC_WORDS */
};
/* what the host passes beside the classify arguments and the tail */
struct ppe_flow_st_args {
    uint32_t *sess;
    unsigned long long *stc;
    uint32_t *tuple_scratch;      /* PPE_FLOW_ST_MAX x 4 words: the batch's tuples when the caller asks for none */
};
/* the detector kernel's arguments, then the session kernel's (csrc/ppe_kernels_flow_portscan_stream.hip):
 * ppe_flow_ps_kargs' three members at their offsets, the list pointers NULL in k and t as in ppe_flow_st_kargs, then the
 * lists, the session records, the counter block under ppe_flow_st_kargs' names */
struct ppe_flow_ps_st_kargs {
    struct ppe_kargs k;
    struct ppe_flow_small_tail t;
    struct ppe_ps_kargs ps;
    uint32_t *fw_idx, *drop_idx, *tile_cnt;
    uint8_t *part8;
    uint32_t *sess;
    unsigned long long *stc;
};
/* the pass behind a rehash: every live flow's record from the old slot arrays to the slot its key took in the new */
struct ppe_flow_st_rehash_kargs {
    const uint32_t *src_keys, *dst_keys;
    const uint32_t *src_sess;
    uint32_t *dst_sess;
    uint32_t nslots, dst_gmask;
};

/* the pass ahead of ppe_flow_age's kernel with monitors and sessions together (csrc/ppe_kernels_flow_stream_attack.hip;
 * DESIGN.md §5.16): the table's current slot arrays, the age kernel's clock, slot 0 of the monitors' slot array */
struct ppe_flow_st_age_kargs {
    const uint32_t *keys;
    const unsigned long long *packed;
    const uint32_t *sess;
    unsigned long long *atk_slots;
    uint64_t now, timeout;
    uint32_t nslots, pad;
};

/* flow-hash steering across GPUs (ppe_steer_partition / ppe_gather_rows / ppe_scatter_rows) */
#define PPE_STEER_MAX_WORLD 16
struct ppe_steer_kargs {
    const uint32_t *verdict;      /* stateless verdict words (PPE_F_L4 in the flags) */
    const uint32_t *flow_hash;
    uint32_t n, world, rank, pad;
    uint32_t *tcount;             /* [tiles][world]: per-tile owner counts, then exclusive offsets into perm */
    uint32_t *perm;               /* [n]: packet indices grouped by owner, ascending within an owner */
    uint32_t *counts;             /* [world] */
};
struct ppe_rows_kargs {
    const uint8_t *src;
    uint8_t *dst;
    const uint32_t *perm;
    uint32_t n, row_bytes;        /* row_bytes: a multiple of 4, <= 256 */
    uint32_t scatter;             /* 0: dst[i] = src[perm[i]]; 1: dst[perm[i]] = src[i] */
    uint32_t pad;
};

struct ppe_tuple_kargs {
    const uint32_t *tuple;    /* n × {sip, dip, sport | dport << 16, proto} */
    const uint32_t *macs;     /* optional n × {dmac lo, dmac hi, smac lo, smac hi} */
    const uint64_t *ts;
    uint32_t n;
    int32_t *hit;
    uint32_t *action;
    const uint32_t *img;
    uint32_t img_words;
    uint32_t default_action;
    uint64_t now;
};

/* The classify kernel's variants (template parameters of ppe_classify_kernel; ppe_launch_info reports them as
 * variant = image mode | tile fetch << 4).
 * Image staging modes:
 *   IMG_GLOBAL  the whole classifier image is read from global memory (L1/L2/MALL-cached)
 *   IMG_LDS     the whole image is staged in LDS
 *   IMG_SPLIT   a prefix [0, lds_words) is staged: header, the top of the BFS tree (every node of the first
 *               lds_iters levels) and, when the prefix reaches them, the leaf lists and the rule records */
#define IMG_GLOBAL 0
#define IMG_LDS 1
#define IMG_SPLIT 2
/* PF: how a wave fetches and walks its tiles.  Register double-buffering (next tile's window, or only its first
 * 16 B, requested before the current tile is processed) and an LDS-DMA next-tile pipeline were measured slower
 * (DESIGN.md §7). */
#define PF_NONE 0   /* one tile per wave, its window loaded at the top of its own iteration */
#define PF_HOIST 1  /* as PF_NONE, but the first tile's loads are issued before the image staging (C1 21.7 us vs 22.2) */
#define PF_MULTI 3  /* split / global images: each wave loads, decodes and walks PPE_MT tiles together
                       (acl_walk_blocks_mt), 4 waves/SIMD with 128 VGPRs, one 1024-thread workgroup per CU and its
                       whole LDS for the image */
#define PF_CUT 5    /* images with cut lists (v7): one tile per wave (8 waves/SIMD), the keys in registers, the bucket
                       groups in LDS, the list entries and ids in LDS (IMG_LDS) or from L2 (IMG_SPLIT) (acl_cut) */

/* How one classifier image is launched under one tuning (csrc/launch_plan.cpp): the kernel variant, its LDS, and
 * every kernel argument that depends on the image and the tuning only.  Computed once per image slot and tuning,
 * never per launch.  Every field is a u32 (ppe/abi.py PLAN_FIELDS mirrors the order). */
struct ppe_plan {
    uint32_t mode;        /* IMG_* */
    uint32_t pipe;        /* PF_* */
    uint32_t block;       /* workgroup size */
    uint32_t lds_bytes;   /* dynamic LDS of the launch (what ppe_launch_info reports for the stateless plan) */
    /* ppe_kargs fields of the same names */
    uint32_t img_words, default_action, lds_words, stage_src, stage_words, lds_blocks, bsec_lds, blk_lds;
    uint32_t off_bsec, off_blocks, max_bdepth, off_crec, off_idtab, crec_lds, idtab_lds;
    uint32_t cut, cut_slc, cut_gbase, cut_fp, cut_ent, cut_epl, cut_div, cut_idrel, cut_gbase_lds, cut_fp_lds,
             cut_ent_lds;
    uint32_t lds_iters, max_depth, max_leaf, root_ks, jump, off_nodes, off_leaf, off_rules, off_resid;
};

#define PPE_CSLOT_WORDS 32
#define PPE_SSLOT_WORDS 8   /* PPE_SC__COUNT */
#define PPE_STM_TRACK 1u
#define PPE_STM_PICKUP 2u
#define PPE_LDS_FIXED 1152u /* classify kernel LDS after the walk keys: 256 counter bins + 32 counters (u32) */
#define PPE_BLOCK 256
/* largest staged classifier image per workgroup (1024-thread workgroups, 2 per CU, each with 25 KB of keys + bins) */
#define PPE_LDS_IMG_MAX (54u * 1024u)

#ifdef __cplusplus
extern "C" {
#endif
/* csrc/launch_plan.cpp (host only: no HIP call, no context, no environment). */
/* the plan of image words[0, n_words) under tuning t; flow != 0: for the flow-table classify kernel (built for the
 * single-tile node walk only).  Returns PPE_OK, or PPE_EINVAL for what is no classifier image */
int ppe_plan_image(const uint32_t *words, uint32_t n_words, const ppe_tuning_t *t, int flow,
                   struct ppe_plan *out);
/* the one place that copies a plan into kernel arguments */
void ppe_plan_apply(struct ppe_kargs *a, const struct ppe_plan *p);
/* batch groups (ppe_kargs.max_groups) of a launch over nbatch batches, at most max_groups */
uint32_t ppe_pick_groups(uint32_t nbatch, uint32_t max_groups);
/* 1: the launch takes the kernels with the port-scan drop mask (PSC): a stateless launch of a context with a table
 * attached whose detector is enabled (portscan_able == 1, dp_portscan.c:238) */
uint32_t ppe_pick_portscan(int flow, int attached, uint32_t able);
/* the pre-pass of a batch of n packets: 1 the one-launch kernel (PPE_PS_K_FUSED) for 1 <= n <= PPE_PS_FUSED_CUTOFF
 * when the table allows it (fused_allowed: not created under PPE_PS_FUSED=0), else 0, the staged launches */
uint32_t ppe_pick_portscan_prepass(uint32_t n, int fused_allowed);
/* 1: the launch takes the kernels with the attack monitors (ATK): a stateless launch of a context with an object
 * attached (ppe_attack_attach), and no other launch */
uint32_t ppe_pick_attack(int flow, int attached);
/* 1: the launch takes the flow-table kernels with the attack monitors (FLOW + ATK) and the post kernel that counts
 * syncount_accum per created flow: a flow-table launch of a context with an object flow-attached
 * (ppe_flow_attack_attach), and no other launch */
uint32_t ppe_pick_attack_flow(int flow, int flow_attached);
/* 1: the flow batch of n packets takes the one-launch kernel: 1 <= n <= PPE_FLOW_SMALL_CUTOFF, the table allows it
 * (small_allowed: not created under PPE_FLOW_SMALL=0, the post-launch failure hook not armed) and no monitors are
 * flow-attached (their syncount count lives in the post kernel); else 0, the two launches */
uint32_t ppe_pick_flow_small(uint32_t n, int small_allowed, int atk_flow_attached);
/* 1: the flow batch of n packets takes the one-launch kernel with the monitors in it (kind 4,
 * csrc/ppe_kernels_flow_small_attack.hip): 1 <= n <= PPE_FLOW_SMALL_ATK_CUTOFF, the table allows it (small_allowed, as
 * above), monitors are flow-attached and the batch comes from ppe_classify_flow_host_ports (ports_call); else 0.
 * ppe_classify_flow's own batches never take it: their two launches with monitors attached are pinned */
uint32_t ppe_pick_flow_small_attack(uint32_t n, int small_allowed, int atk_flow_attached, int ports_call);
/* 1: the ppe_defrag batch of n fragments takes the one-launch kernel: 1 <= n <= PPE_DEFRAG_SMALL_CUTOFF, the table
 * allows it (small_allowed: not created under PPE_DEFRAG_SMALL=0) and the admission look-back's failure hook
 * (PPE_DF_LOOK_FAIL) is not armed; else 0, the six launches */
uint32_t ppe_pick_defrag_small(uint32_t n, int small_allowed, int look_fail_armed);
/* the planner's general form, which ppe_defrag calls: the one launch for 1 <= n <= upto (clamped to
 * PPE_DEFRAG_SMALL_BLOCK) unless the hook is armed; upto is the table's, from PPE_DEFRAG_SMALL at ppe_defrag_create
 * (`value`: its integer, -1 when unset): unset or 1 the cutoff, 0 none, N > 1 min(N, PPE_DEFRAG_SMALL_BLOCK), a
 * diagnostic for measuring and testing the kernel past the cutoff */
uint32_t ppe_pick_defrag_small_upto(uint32_t n, uint32_t upto, int look_fail_armed);
uint32_t ppe_defrag_small_upto_from_env(int value);
/* the one-launch defrag kernel (csrc/ppe_defrag_small.hip): one workgroup of PPE_DEFRAG_SMALL_BLOCK threads over the
 * batch in `args` (csrc/ppe_defrag.hip's argument block, `bytes` its size).  Returns hipError_t */
int ppe_launch_defrag_small(const void *args, uint32_t bytes, void *stream);
/* how a flow batch of n packets runs with respect to the port-scan detector: PPE_FPS_PLAIN today's kernels (no table
 * flow-attached, or its detector off: portscan_able == 0), PPE_FPS_KERNEL the one-launch kernel with the detector
 * inside (1 <= n <= PPE_FLOW_PS_MAX), PPE_FPS_REFUSE a larger batch (PPE_ENOTSUP before anything is touched) */
enum { PPE_FPS_PLAIN = 0, PPE_FPS_KERNEL = 1, PPE_FPS_REFUSE = 2 };
uint32_t ppe_pick_flow_portscan(uint32_t n, int flow_attached, uint32_t able);
/* the detector and the attack monitors on one flow batch.  fps: ppe_pick_flow_portscan's answer.  PPE_FPC_NONE: not the
 * combination (fps PLAIN, or no monitors flow-attached): as before; PPE_FPC_KERNEL: the combined kernel
 * (csrc/ppe_kernels_flow_portscan_attack.hip: fps KERNEL, monitors, combine on); PPE_FPC_REFUSE: refuse (monitors
 * flow-attached and fps != PLAIN, with combine off or fps REFUSE) */
enum { PPE_FPC_NONE = 0, PPE_FPC_KERNEL = 1, PPE_FPC_REFUSE = 2 };
uint32_t ppe_pick_flow_combined(uint32_t fps, int atk_flow_attached, uint32_t combine_on);
/* how a flow batch of n packets runs with respect to the TCP session machine: PPE_FST_PLAIN today's kernels (sessions
 * not attached, or tracking off), PPE_FST_KERNEL the one-launch kernel with the session phase (1 <= n <=
 * PPE_FLOW_ST_MAX), PPE_FST_REFUSE (PPE_ENOTSUP before anything is touched): a larger batch, a configuration other than
 * {midstream 0, async_oneside 0, reasm 0}, or a port-scan table or monitors flow-attached as well */
enum { PPE_FST_PLAIN = 0, PPE_FST_KERNEL = 1, PPE_FST_REFUSE = 2 };
uint32_t ppe_pick_flow_stream(uint32_t n, int attached, uint32_t track, uint32_t midstream, uint32_t async_oneside,
                              uint32_t reasm, int ps_flow_attached, int atk_flow_attached);
/* the one-launch flow kernel with the session phase (csrc/ppe_kernels_flow_stream.hip): one workgroup of
 * PPE_FLOW_ST_BLOCK threads, 1 <= a->batch[0].n <= PPE_FLOW_ST_MAX, a->batch[0].stride >= 144; a->flow.upd_wgs must be 0.
 * Returns hipError_t */
int ppe_launch_flow_stream(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                           const struct ppe_flow_st_args *st, int mode, void *stream, void *ev_start, void *ev_stop);
/* the session records' pass behind the flow rehash launch (same file).  Returns hipError_t */
int ppe_launch_flow_stream_rehash(const struct ppe_flow_st_rehash_kargs *a, uint32_t grid, void *stream);
/* monitors flow-attached and sessions attached on one batch (ppe_flow_stream_monitors): as ppe_pick_flow_stream, with
 * PPE_FST_KERNEL_ATK the one-launch kernel with both inside (kind 6: monitors_on 1, monitors flow-attached, no port-scan
 * table flow-attached, the one configuration, 1 <= n <= PPE_FLOW_ST_MAX).  monitors_on 0: ppe_pick_flow_stream's
 * answer, whatever else is set; sessions not attached or tracking off: PPE_FST_PLAIN */
#define PPE_FST_KERNEL_ATK 3u
uint32_t ppe_pick_flow_stream_monitors(uint32_t n, int attached, uint32_t track, uint32_t midstream,
                                       uint32_t async_oneside, uint32_t reasm, int ps_flow_attached,
                                       int atk_flow_attached, uint32_t monitors_on);
/* the one-launch flow kernel with the session phase and the attack monitors (csrc/ppe_kernels_flow_stream_attack.hip):
 * as ppe_launch_flow_stream; a->fatk_st and a->fatk_slots must be set.  Returns hipError_t */
int ppe_launch_flow_stream_attack(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                                  const struct ppe_flow_st_args *st, int mode, void *stream, void *ev_start,
                                  void *ev_stop);
/* StreamTcp_Flow_ResRelease's syncount_accum decrements for the flows the age kernel behind it deletes (same file).
 * Returns hipError_t */
int ppe_launch_flow_stream_age_release(const struct ppe_flow_st_age_kargs *a, uint32_t grid, void *stream);
/* the port-scan detector and the sessions on one batch (ppe_flow_stream_portscan): everything
 * ppe_pick_flow_stream_monitors takes, the table's portscan_able, the new switch and ppe_flow_combine's.  portscan_on 0,
 * or no table flow-attached: ppe_pick_flow_stream_monitors' answer.  On, able != 1: the detector is off, so its answer
 * as if no table were flow-attached (kinds 5 / 6).  On, able 1: sessions not attached or tracking off PPE_FST_PLAIN (the
 * detector's own planners decide); the one configuration and 1 <= n <= min(PPE_FLOW_PS_MAX, PPE_FLOW_ST_MAX):
 * PPE_FST_KERNEL_PS without monitors flow-attached (kind 7), PPE_FST_KERNEL_PS_ATK with them when monitors_on and
 * combine_on are both 1 (kind 8); everything else PPE_FST_REFUSE */
#define PPE_FST_KERNEL_PS 4u
#define PPE_FST_KERNEL_PS_ATK 5u
uint32_t ppe_pick_flow_stream_portscan(uint32_t n, int attached, uint32_t track, uint32_t midstream,
                                       uint32_t async_oneside, uint32_t reasm, int ps_flow_attached,
                                       int atk_flow_attached, uint32_t monitors_on, uint32_t able, uint32_t portscan_on,
                                       uint32_t combine_on);
/* the one-launch flow kernel with the detector inside and the session phase behind it
 * (csrc/ppe_kernels_flow_portscan_stream.hip): as ppe_launch_flow_portscan and ppe_launch_flow_stream together, 1 <=
 * a->batch[0].n <= min(PPE_FLOW_PS_MAX, PPE_FLOW_ST_MAX), a->batch[0].stride >= 144.  Returns hipError_t */
int ppe_launch_flow_stream_portscan(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                                    const struct ppe_ps_kargs *ps, const struct ppe_flow_st_args *st, int mode,
                                    void *stream, void *ev_start, void *ev_stop);
/* the same with the attack monitors in it (csrc/ppe_kernels_flow_portscan_attack_stream.hip): a->fatk_st and
 * a->fatk_slots must be set.  Returns hipError_t */
int ppe_launch_flow_stream_portscan_attack(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                                           const struct ppe_ps_kargs *ps, const struct ppe_flow_st_args *st, int mode,
                                           void *stream, void *ev_start, void *ev_stop);
/* The machine itself on the host, as the kernel compiles it (csrc/ppe_stream_session_dev.h, csrc/ppe_stream_session.cpp):
 * one StreamTcpPacket step on a 16-word session record (the device layout).  pkt = {th_flags, seq, ack, window,
 * payload_len, window-scale shift byte or 0xff without the option, toclient 0/1}; counters (64 words, may be NULL) get
 * the fields counted.  Returns 0 or the reason.  No context, no device: the CPU tests hold it against the serial model
 * (an internal helper like the planner's, not part of the public headers) */
uint32_t ppe_stream_session_step(uint32_t record[16], const uint32_t pkt[7], uint64_t *counters);
/* the monitors' set / tick / clear kernel (csrc/ppe_attack.hip), stream-ordered.  Returns hipError_t */
int ppe_launch_attack_ctl(const struct ppe_atk_kargs *a, void *stream);
/* one kernel of the port-scan pre-pass (csrc/ppe_portscan.hip), grid sized from the arguments.  Returns hipError_t */
int ppe_launch_portscan(int kind, const struct ppe_ps_kargs *a, void *stream);

/* Launch the classify kernel. grid = workgroups (persistent). Returns hipError_t.  mode: IMG_*, pipe: PF_* */
int ppe_launch_classify(const struct ppe_kargs *a, uint32_t grid, int mode, int pipe, int block, int flow,
                        void *stream, void *ev_start, void *ev_stop);
/* flow-table phases after a flow-mode classify launch (stream order): claim, resolve, finalize (+ revoke in its
 * workgroup 0 when the pool overflows) */
enum { PPE_FLOW_K_POST = 0, PPE_FLOW_K_AGE, PPE_FLOW_K_REHASH };
int ppe_launch_flow(int kind, const struct ppe_flow_kargs *a, uint32_t grid, void *stream);
/* the one-launch flow kernel over the image placement `mode` (csrc/ppe_kernels_flow_small.hip): one workgroup of
 * PPE_FLOW_SMALL_BLOCK threads; a->flow.upd_wgs must be 0.  Returns hipError_t */
int ppe_launch_flow_small(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t, int mode, void *stream,
                          void *ev_start, void *ev_stop);
/* the same with the attack monitors in the classify phase and the syncount_accum count in finalize
 * (csrc/ppe_kernels_flow_small_attack.hip): a->fatk_st and a->fatk_slots must be set, 1 <= a->batch[0].n <=
 * PPE_FLOW_SMALL_CUTOFF (the kernel's own bound; the planner stops at PPE_FLOW_SMALL_ATK_CUTOFF).  Returns hipError_t */
int ppe_launch_flow_small_attack(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t, int mode, void *stream,
                                 void *ev_start, void *ev_stop);
/* the one-launch flow kernel with the port-scan detector inside (csrc/ppe_kernels_flow_portscan.hip): one workgroup of
 * PPE_FLOW_PS_BLOCK threads, a->batch[0].n <= PPE_FLOW_PS_MAX; a->flow.upd_wgs must be 0.  Returns hipError_t */
int ppe_launch_flow_portscan(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                             const struct ppe_ps_kargs *ps, int mode, void *stream, void *ev_start, void *ev_stop);
/* the same with the attack monitors in the classify phase and the syncount_accum count in finalize
 * (csrc/ppe_kernels_flow_portscan_attack.hip): a->fatk_st and a->fatk_slots must be set.  Returns hipError_t */
int ppe_launch_flow_portscan_attack(const struct ppe_kargs *a, const struct ppe_flow_small_tail *t,
                                    const struct ppe_ps_kargs *ps, int mode, void *stream, void *ev_start,
                                    void *ev_stop);
#define PPE_FLOW_BLOCK 256      /* flow kernels' workgroup size */
/* steering: 0 count, 1 scan (one workgroup), 2 scatter the permutation; rows: gather / scatter of fixed rows */
int ppe_launch_steer(int phase, const struct ppe_steer_kargs *a, uint32_t grid, void *stream);
int ppe_launch_rows(const struct ppe_rows_kargs *a, uint32_t grid, void *stream);
#define PPE_FLOW_BLOCK_WAVES 4u /* waves (tiles in flight) per flow-kernel workgroup */
int ppe_classify_occupancy(uint32_t lds_words, int mode, int pipe, int block);
uint32_t ppe_classify_fixed_lds(int block, int pipe, int mode);
uint32_t ppe_flow_lds_extra(void);  /* classify LDS of a flow-table launch beyond the stateless kernel's (buckets) */
uint32_t ppe_flow_waves(void);      /* waves per SIMD of the flow-table classify kernel */
int ppe_classify_occupancy_flow(uint32_t lds_words, int mode, int block);  /* key slots (node walks only) + counter bins */
int ppe_launch_acl_tuples(const struct ppe_tuple_kargs *a, uint32_t grid, int lds_img, void *stream);
#ifdef __cplusplus
}
#endif

#endif
