/*
 * launch_plan.cpp — how a classifier image is launched: a pure function of (image, tuning, stateless / flow-table).
 *
 * Host only: no HIP call, no context, no environment.  The engine computes a plan when an image is uploaded or the
 * tuning changes and keeps it per image slot (ppe_engine.hip); tests/test_launch_plan.py checks it on the CPU against
 * recorded plans.  The LDS sizes of the kernels (ppe_classify_fixed_lds, ppe_flow_lds_extra, ppe_flow_waves) stay in
 * ppe_kernels.hip, whose macros an experimental build overrides (make variant).
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "ppe_hip.h"
#include "ppe_image.h"
#include "ppe_internal.h"

namespace {

// LDS left for the image per workgroup when the CU holds 2048 / block workgroups (32 waves; a flow-table launch:
// the waves per CU its kernel is compiled for): 160 KiB shared, minus the per-wave walk keys and counter bins
// (flow-table launches: and the owner-update buckets), and the 1-KB rounding of the staged image
uint32_t image_budget(uint32_t block, int mode, bool flow = false) {
    const uint32_t waves_cu = flow ? std::min(32u, std::max(block / 64u, 4u * ppe_flow_waves())) : 32u;
    const uint32_t per_wg = (160u * 1024u) / std::max(1u, waves_cu / (block / 64u));
    const uint32_t fixed = ppe_classify_fixed_lds((int)block, PF_HOIST, mode) + 1024u + (flow ? ppe_flow_lds_extra() : 0u);
    return per_wg > fixed ? per_wg - fixed : 0u;
}

// Image placement, tile fetch, workgroup size and LDS offsets, into p (zeroed but for the ~0u "from global memory"
// offsets).  lds_nodes: the binary nodes a single-tile walk finds in its staged prefix.
// single: the plan for the single-tile node-walk kernel only (the flow-table classify kernel is built for it: its
// key slots and node prefix), never the multi-tile or cut-list plans
void stage_plan(const ppe_tuning_t &tune, const uint32_t *img, uint32_t n_words, bool single, ppe_plan &p,
                uint32_t &lds_nodes) {
    const uint32_t pf = tune.pipeline == 1 ? PF_NONE : PF_HOIST;
    // the single-tile walk reads the binary nodes only: what it stages "whole" is the image before the block section
    const uint32_t all_words = img[PPE_IMG_W_OFFCUT] ? img[PPE_IMG_W_OFFCUT] : n_words;  // tree part
    const uint32_t off_bsec = img[PPE_IMG_W_OFFBSEC], off_blocks = img[PPE_IMG_W_OFFBLOCKS];
    const uint32_t n_blocks = img[PPE_IMG_W_NBLOCKS];
    const uint32_t words = off_bsec, bytes = words * 4u;
    p.mode = IMG_GLOBAL;
    p.pipe = pf;
    p.block = tune.block ? tune.block : 1024u;
    // the multi-tile walk reads the 2-level blocks: whole image in LDS, else the block jump table and the first
    // block levels (breadth-first), else global
    const uint32_t off_crec = img[PPE_IMG_W_OFFCREC], off_idtab = img[PPE_IMG_W_OFFIDTAB];
    constexpr uint32_t bbytes = 32u;
    auto mt_plan = [&](uint32_t budget) {
        const uint32_t bjt = 4u * (off_blocks - off_bsec);
        if (off_crec && (all_words - off_bsec) * 4u <= budget) {
            // compact image (v6): the block walk needs only the block section and the compact records after it, so
            // the whole walk is LDS-resident when they fit (C2 / C4: 4,096 rules, ~140 KB)
            p.mode = IMG_LDS;
            p.stage_src = off_bsec;
            p.lds_words = p.stage_words = all_words - off_bsec;
            p.lds_blocks = n_blocks;
            p.bsec_lds = 0;
            p.blk_lds = 4u * (off_blocks - off_bsec);
            p.crec_lds = 4u * (off_crec - off_bsec);
            if (off_idtab) p.idtab_lds = 4u * (off_idtab - off_bsec);
        } else if (!off_crec && all_words * 4u <= budget) {
            p.mode = IMG_LDS;
            p.lds_words = p.stage_words = all_words;
            p.lds_blocks = n_blocks;
            p.bsec_lds = 4u * off_bsec;
            p.blk_lds = 4u * off_blocks;
        } else if (budget >= bjt + bbytes * 64u) {
            p.mode = IMG_SPLIT;
            p.lds_blocks = std::min(n_blocks, (budget - bjt) / bbytes);
            p.stage_src = off_bsec;
            p.stage_words = (off_blocks - off_bsec) + (bbytes / 4u) * p.lds_blocks;
            p.bsec_lds = 0;
            p.blk_lds = bjt;
        }
    };
    // the cut lists (image v8): the bucket groups in LDS (the smallest workgroup whose share at 32 waves per CU holds
    // them; the entries too when they fit beside them), the entries read from L2 otherwise; one tile per wave at 8
    // waves per SIMD.  lds_image = 0: both from global memory.
    const uint32_t off_cut = img[PPE_IMG_W_OFFCUT];
    auto cut_plan = [&]() {
        const uint32_t *h = img + off_cut;
        const uint32_t grp_bytes = 4u * (h[5] - h[4]);  // slices, bases and fingerprints (the L2-entry plan's LDS)
        const uint32_t all_words = h[5] - h[4] + 32u * h[11] +  // ... to the end of the entry lines (and the ids)
                                   (h[0] & PPE_CUT_LINES ? 0u : h[0] & PPE_CUT_IDS16 ? (h[2] + 1u) / 2u : h[2]);
        p.pipe = PF_CUT;
        p.mode = IMG_GLOBAL;
        p.block = tune.block ? tune.block : 1024u;
        p.cut_ent_lds = ~0u;  // (entry lines from global memory unless staged below)
        if (!tune.lds_image) return;
        auto budget = [&](uint32_t b) {  // (no key slots: the keys stay in registers)
            const uint32_t per_wg = (160u * 1024u) / std::max(1u, 32u / (b / 64u));
            const uint32_t fixed = ppe_classify_fixed_lds((int)b, PF_CUT, IMG_LDS) + 1024u;
            return per_wg > fixed ? per_wg - fixed : 0u;
        };
        if (!tune.block)
            for (uint32_t b : {256u, 512u, 1024u})
                if (4u * all_words <= budget(b) || (b == 1024u && grp_bytes <= budget(b))) {
                    p.block = b;
                    break;
                }
        const uint32_t bud = budget(p.block);
        if (grp_bytes > bud) return;  // (groups larger than the share: global)
        p.stage_src = h[4];
        p.cut_gbase_lds = 4u * (h[8] - h[4]);
        p.cut_fp_lds = 4u * (h[9] - h[4]);
        // everything in LDS (IMG_LDS: the dense layout only, the kernel's entry addressing assumes it)
        if (4u * all_words <= bud && !(h[0] & PPE_CUT_LINES)) {
            p.mode = IMG_LDS;
            p.stage_words = all_words;
            p.cut_ent_lds = 4u * (h[5] - h[4]);
        } else {  // slices, bases and fingerprints in LDS, the entry lines from L2 (IMG_SPLIT)
            p.mode = IMG_SPLIT;
            p.stage_words = h[5] - h[4];
        }
        p.lds_words = p.stage_words;
    };
    if (!single && off_cut && tune.pipeline == 5) {
        cut_plan();
        return;
    }
    if (!tune.lds_image) {
        if (!tune.block) p.block = 256;
        if (!single && (tune.pipeline == 3 || (tune.pipeline == 0 && !tune.block))) {  // PF_MULTI, global image
            p.pipe = PF_MULTI;
            p.block = 1024u;
        }
        return;
    }
    // the whole image in LDS: the smallest workgroup (most copies per CU) whose share holds it (a node walk reads
    // the part before the block section)
    const uint32_t lds_bytes = bytes;
    if (!tune.block) {
        for (uint32_t b : {256u, 512u, 1024u}) {
            if (lds_bytes <= image_budget(b, IMG_LDS, single)) {
                p.block = b;
                break;
            }
        }
    }
    uint32_t budget = image_budget(p.block, IMG_LDS, single);
    const bool fits = lds_bytes <= budget;
    // images that do not fit whole: the cut lists when the image has them (C2 / C3 / C4), else PF_MULTI
    // (1024-thread workgroups, one per CU, with the CU's whole LDS for the image prefix: C2 / C3 / C4 step 27.2 /
    // 52.1 / 27.3 -> 23.6 / 42.8 / 22.7 us against the single-tile node walk)
    if (!single && off_cut && tune.pipeline == 0 && !fits && !tune.block) {
        cut_plan();
        return;
    }
    if (!single && (tune.pipeline == 3 || (tune.pipeline == 0 && !fits && !tune.block))) {
        p.pipe = PF_MULTI;
        p.block = 1024u;
        const uint32_t fixed = ppe_classify_fixed_lds((int)p.block, PF_MULTI, IMG_SPLIT) + 1024u;  // no key slots
        mt_plan(160u * 1024u - fixed);  // one workgroup per CU: all of its LDS
        return;
    }
    const uint32_t off_resid = img[PPE_IMG_W_OFFRESID], off_rules = img[PPE_IMG_W_OFFRULES];
    const uint32_t n_nodes = img[PPE_IMG_W_NNODES], off_nodes = img[PPE_IMG_W_OFFNODES];
    if (fits) {
        p.mode = IMG_LDS;
        p.lds_words = p.stage_words = words;
        return;
    }
    budget = image_budget(p.block, IMG_SPLIT, single);  // node walks of a partly staged image keep their key slots
    if (off_resid * 4u <= budget) {  // nodes, leaf lists and rule records; residual records from global
        p.mode = IMG_SPLIT;
        p.lds_words = off_resid;
        lds_nodes = n_nodes;
    } else if (off_rules * 4u <= budget) {  // every node and leaf list; rule records from global (L2)
        p.mode = IMG_SPLIT;
        p.lds_words = off_rules;
        lds_nodes = n_nodes;
    } else if (budget >= 4u * (off_nodes + PPE_NODE_WORDS * 64u)) {  // header, jump table, top of the BFS forest
        p.mode = IMG_SPLIT;
        lds_nodes = std::min(n_nodes, (budget / 4u - off_nodes) / PPE_NODE_WORDS);
        p.lds_words = off_nodes + PPE_NODE_WORDS * lds_nodes;
    }
    p.stage_words = p.lds_words;  // single-tile walks stage a prefix from word 0
}

// Walk levels (node reads) whose nodes all lie in the first lds_nodes nodes of the image
uint32_t levels_within(const uint32_t *words, uint32_t lds_nodes) {
    // BFS node order: the nodes of depth <= d are exactly [0, level_end[d])
    std::vector<uint32_t> le;
    const uint32_t nn = words[PPE_IMG_W_NNODES], on = words[PPE_IMG_W_OFFNODES];
    std::vector<uint8_t> depth(nn, 0);  // every root of the forest (jump root: several) has depth 0
    for (uint32_t k = 0; k < nn; ++k) {
        const uint32_t *nd = words + on + PPE_NODE_WORDS * k;
        if (nd[0] != PPE_LEAF_THR) {  // children: byte offsets from the image start
            depth[(nd[1] / 4u - on) / PPE_NODE_WORDS] = (uint8_t)(depth[k] + 1u);
            depth[(nd[2] / 4u - on) / PPE_NODE_WORDS] = (uint8_t)(depth[k] + 1u);
        }
        if (le.size() <= depth[k]) le.resize(depth[k] + 1u, 0u);
        le[depth[k]] = k + 1u;
    }
    uint32_t L = 0;
    while (L < le.size() && le[L] <= lds_nodes) ++L;
    return L;
}

}  // namespace

extern "C" {

int ppe_plan_image(const uint32_t *words, uint32_t n_words, const ppe_tuning_t *t, int flow, struct ppe_plan *out) {
    if (!words || !t || !out || n_words < PPE_IMG_HDR_WORDS || words[0] != PPE_IMG_MAGIC ||
        words[1] != PPE_IMG_VERSION)
        return PPE_EINVAL;
    if (t->block != 0 && t->block != 256 && t->block != 512 && t->block != 1024) return PPE_EINVAL;
    ppe_plan p;
    std::memset(&p, 0, sizeof p);
    p.crec_lds = p.idtab_lds = ~0u;  // compact records / index table: read from global memory
    uint32_t lds_nodes = 0;
    stage_plan(*t, words, n_words, flow != 0, p, lds_nodes);
    // (what ppe_launch_classify allocates: the kernel's fixed LDS and the staged words rounded to 1 KB)
    p.lds_bytes = ppe_classify_fixed_lds((int)p.block, (int)p.pipe, (int)p.mode) + (flow ? ppe_flow_lds_extra() : 0u) +
                  (p.mode ? ((p.stage_words * 4u + 1023u) & ~1023u) : 0u);
    p.img_words = n_words;
    p.default_action = words[PPE_IMG_W_DEFACT];
    p.off_bsec = words[PPE_IMG_W_OFFBSEC];
    p.off_blocks = words[PPE_IMG_W_OFFBLOCKS];
    p.max_bdepth = words[PPE_IMG_W_MAXBDEPTH];
    p.off_crec = words[PPE_IMG_W_OFFCREC];
    p.off_idtab = words[PPE_IMG_W_OFFIDTAB];
    if (p.pipe == PF_CUT) {  // (image v8 cut lists: header at PPE_IMG_W_OFFCUT)
        const uint32_t *h = words + words[PPE_IMG_W_OFFCUT];
        p.cut = h[0];
        p.cut_slc = h[4];
        p.cut_ent = h[5];
        p.cut_epl = h[7];
        p.cut_div = h[10];
        p.cut_idrel = (h[0] & PPE_CUT_LINES) ? 0u : 4u * (h[12] - h[5]);
        p.cut_gbase = h[8];
        p.cut_fp = h[9];
    }
    p.max_depth = words[PPE_IMG_W_MAXDEPTH];
    p.max_leaf = words[PPE_IMG_W_MAXLEAF];
    p.root_ks = words[PPE_IMG_W_ROOTKS];
    p.jump = words[PPE_IMG_W_JUMP];
    p.off_nodes = words[PPE_IMG_W_OFFNODES];
    if (p.mode == IMG_LDS) {
        p.lds_iters = p.max_depth + 1u;
    } else if (p.mode == IMG_SPLIT) {  // node reads 0..L-1 only visit depths < L: all inside the staged prefix
        p.lds_iters = std::min(levels_within(words, lds_nodes), p.max_depth + 1u);
    }
    p.off_leaf = words[PPE_IMG_W_OFFLEAF];
    p.off_rules = words[PPE_IMG_W_OFFRULES];
    p.off_resid = words[PPE_IMG_W_OFFRESID];
    *out = p;
    return PPE_OK;
}

void ppe_plan_apply(struct ppe_kargs *a, const struct ppe_plan *p) {
    a->img_words = p->img_words;
    a->default_action = p->default_action;
    a->lds_words = p->lds_words;
    a->stage_src = p->stage_src;
    a->stage_words = p->stage_words;
    a->lds_blocks = p->lds_blocks;
    a->bsec_lds = p->bsec_lds;
    a->blk_lds = p->blk_lds;
    a->off_bsec = p->off_bsec;
    a->off_blocks = p->off_blocks;
    a->max_bdepth = p->max_bdepth;
    a->off_crec = p->off_crec;
    a->off_idtab = p->off_idtab;
    a->crec_lds = p->crec_lds;
    a->idtab_lds = p->idtab_lds;
    a->cut = p->cut;
    a->cut_slc = p->cut_slc;
    a->cut_gbase = p->cut_gbase;
    a->cut_fp = p->cut_fp;
    a->cut_ent = p->cut_ent;
    a->cut_epl = p->cut_epl;
    a->cut_div = p->cut_div;
    a->cut_idrel = p->cut_idrel;
    a->cut_gbase_lds = p->cut_gbase_lds;
    a->cut_fp_lds = p->cut_fp_lds;
    a->cut_ent_lds = p->cut_ent_lds;
    a->lds_iters = p->lds_iters;
    a->max_depth = p->max_depth;
    a->max_leaf = p->max_leaf;
    a->root_ks = p->root_ks;
    a->jump = p->jump;
    a->off_nodes = p->off_nodes;
    a->off_leaf = p->off_leaf;
    a->off_rules = p->off_rules;
    a->off_resid = p->off_resid;
}

// Batch groups: the kernel splits its waves into min(batches, max_groups) groups, group g taking batches g, g + G,
// ...; when G does not divide the batch count the last round leaves groups idle (20 batches at G = 8: the last
// 4 run on half the grid; C3 / C4 ring step +12 %, profiles/r3_ab_runs.md r4l).  Take the power-of-two G up to the
// cap (or the batch count itself when smaller) with the least work-slot time, ceil(batches / G) x G batch slots
// weighted by the per-batch cost of G groups (1 group 1.10, 2 groups 1.02, more 1.00: C1 per-batch 20.2 / 18.7 /
// 18.3 us at 1 / 2 / >= 4 groups); ties go to the larger G.  20 batches -> 4 groups, 32 -> 8, 33 -> 2.
uint32_t ppe_pick_groups(uint32_t nb, uint32_t max_groups) {
    const uint32_t gmax = std::max(1u, std::min(max_groups, nb));
    auto cost = [&](uint32_t g) {
        return (double)((nb + g - 1u) / g * g) * (g == 1u ? 1.10 : g == 2u ? 1.02 : 1.0);
    };
    uint32_t best = gmax;
    double cbest = cost(gmax);
    for (uint32_t g = 1u << (31 - __builtin_clz(gmax)); g >= 1u; g >>= 1) {
        if (g == gmax) continue;
        if (cost(g) < cbest - 1e-9) {
            best = g;
            cbest = cost(g);
        }
    }
    return best;
}

uint32_t ppe_pick_portscan(int flow, int attached, uint32_t able) {
    return (!flow && attached && able == 1u) ? 1u : 0u;  // portscan_able != 1: DECODE_OK at once (dp_portscan.c:238-241)
}

uint32_t ppe_pick_portscan_prepass(uint32_t n, int fused_allowed) {
    return (fused_allowed && n >= 1u && n <= PPE_PS_FUSED_CUTOFF) ? 1u : 0u;
}

uint32_t ppe_pick_attack(int flow, int attached) {
    return (!flow && attached) ? 1u : 0u;  // the monitors sit in the decoders (decode-ipv4.c:141-149, decode-tcp.c:162-173)
}

// the same monitors ahead of FlowFind, with syncount_accum counted per created flow (FlowAdd, flow.c:151-154): only a
// flow-table launch of a context with an object attached for that path (ppe_flow_attack_attach)
uint32_t ppe_pick_attack_flow(int flow, int flow_attached) {
    return (flow && flow_attached) ? 1u : 0u;
}

// one launch of one workgroup for a small flow batch (csrc/ppe_kernels_flow_small.hip): up to the measured cutoff,
// unless the table was created without it or monitors are flow-attached (FLOW + ATK keeps the two launches: its
// syncount_accum count lives in the post kernel)
uint32_t ppe_pick_flow_small(uint32_t n, int small_allowed, int atk_flow_attached) {
    return (n >= 1u && n <= PPE_FLOW_SMALL_CUTOFF && small_allowed && !atk_flow_attached) ? 1u : 0u;
}

// the same kernel with the monitors in it (csrc/ppe_kernels_flow_small_attack.hip, launch kind 4): up to its own measured
// cutoff, for a batch of ppe_classify_flow_host_ports with monitors flow-attached.  ppe_classify_flow's own batches
// (ports_call 0) keep the two launches
uint32_t ppe_pick_flow_small_attack(uint32_t n, int small_allowed, int atk_flow_attached, int ports_call) {
    static_assert(PPE_FLOW_SMALL_ATK_CUTOFF >= 64u && PPE_FLOW_SMALL_ATK_CUTOFF % 64u == 0u &&
                  PPE_FLOW_SMALL_ATK_CUTOFF <= PPE_FLOW_SMALL_CUTOFF, "a multiple of 64 inside the kernel's own bound");
    return (n >= 1u && n <= PPE_FLOW_SMALL_ATK_CUTOFF && small_allowed && atk_flow_attached && ports_call) ? 1u : 0u;
}

// one launch of one workgroup for a small fragment batch (csrc/ppe_defrag_small.hip): up to `upto` fragments (the
// table's: the measured cutoff, 0 under PPE_DEFRAG_SMALL=0, the diagnostic PPE_DEFRAG_SMALL=N's value; never past the
// workgroup), unless the look-back failure hook is armed (one workgroup has no look-back to fail).  The one decision
// point: ppe_defrag calls this form with its table's value.
uint32_t ppe_pick_defrag_small_upto(uint32_t n, uint32_t upto, int look_fail_armed) {
    if (upto > (uint32_t)PPE_DEFRAG_SMALL_BLOCK) upto = (uint32_t)PPE_DEFRAG_SMALL_BLOCK;
    return (n >= 1u && n <= upto && !look_fail_armed) ? 1u : 0u;
}

// the same for a table at its default: up to the measured cutoff when the table allows it
uint32_t ppe_pick_defrag_small(uint32_t n, int small_allowed, int look_fail_armed) {
    return ppe_pick_defrag_small_upto(n, small_allowed ? PPE_DEFRAG_SMALL_CUTOFF : 0u, look_fail_armed);
}

// what PPE_DEFRAG_SMALL (its integer value, or -1 when unset) makes of a new table's `upto`: unset or 1 the cutoff, 0
// none (the A/B switch), N > 1 min(N, the workgroup) (diagnostic)
uint32_t ppe_defrag_small_upto_from_env(int value) {
    if (value == 0) return 0u;
    if (value < 0 || value == 1) return PPE_DEFRAG_SMALL_CUTOFF;
    return (uint32_t)value < (uint32_t)PPE_DEFRAG_SMALL_BLOCK ? (uint32_t)value : (uint32_t)PPE_DEFRAG_SMALL_BLOCK;
}

// the port-scan detector on the flow-table path (csrc/ppe_kernels_flow_portscan.hip): with a table flow-attached and its
// detector on, a batch of up to one workgroup's worth of packets takes the kernel with the detector inside; a larger one
// is refused (whether a packet reaches the detector depends on verdicts of earlier packets of the batch: a grid-wide form
// is not built).  Nothing flow-attached, or portscan_able == 0 (dp_portscan.c:238): today's kernels at every size
uint32_t ppe_pick_flow_portscan(uint32_t n, int flow_attached, uint32_t able) {
    if (!flow_attached || able != 1u) return PPE_FPS_PLAIN;
    return n <= PPE_FLOW_PS_MAX ? PPE_FPS_KERNEL : PPE_FPS_REFUSE;
}

// the detector and the attack monitors both flow-attached (csrc/ppe_kernels_flow_portscan_attack.hip): the reference's
// whole path in one launch, for a context that asked for it (ppe_flow_combine; off, the batch is refused as it always
// was); a batch the detector's kernel cannot take is refused with the monitors as without them.  fps PLAIN (no table, or
// portscan_able == 0) or no monitors: not the combination, whatever the switch says
uint32_t ppe_pick_flow_combined(uint32_t fps, int atk_flow_attached, uint32_t combine_on) {
    if (fps == PPE_FPS_PLAIN || !atk_flow_attached) return PPE_FPC_NONE;
    return (fps == PPE_FPS_KERNEL && combine_on == 1u) ? PPE_FPC_KERNEL : PPE_FPC_REFUSE;
}

// the TCP session machine behind the flow table (csrc/ppe_kernels_flow_stream.hip; ppe_flow_stream_attach): it is built
// for the one configuration in which StreamTcp is a pure verdict (midstream 0, async_oneside 0, reasm 0), one workgroup
// per batch, and neither the detector nor the monitors on the same batch.  Sessions not attached or tracking off: the
// plain kernels, whatever else is set
uint32_t ppe_pick_flow_stream(uint32_t n, int attached, uint32_t track, uint32_t midstream, uint32_t async_oneside,
                              uint32_t reasm, int ps_flow_attached, int atk_flow_attached) {
    if (!attached || track != 1u) return PPE_FST_PLAIN;
    if (midstream != 0u || async_oneside != 0u || reasm != 0u) return PPE_FST_REFUSE;
    if (ps_flow_attached || atk_flow_attached) return PPE_FST_REFUSE;
    return n <= PPE_FLOW_ST_MAX ? PPE_FST_KERNEL : PPE_FST_REFUSE;
}

// the same with the context's switch for monitors and sessions on one batch (ppe_flow_stream_monitors;
// csrc/ppe_kernels_flow_stream_attack.hip): off, ppe_pick_flow_stream's answer; on, monitors flow-attached beside the
// sessions take the kernel with both inside, and everything else is as without the switch (a port-scan table
// flow-attached as well, whatever its `able`, is still refused)
uint32_t ppe_pick_flow_stream_monitors(uint32_t n, int attached, uint32_t track, uint32_t midstream,
                                       uint32_t async_oneside, uint32_t reasm, int ps_flow_attached,
                                       int atk_flow_attached, uint32_t monitors_on) {
    if (monitors_on != 1u || !atk_flow_attached)
        return ppe_pick_flow_stream(n, attached, track, midstream, async_oneside, reasm, ps_flow_attached, atk_flow_attached);
    const uint32_t r = ppe_pick_flow_stream(n, attached, track, midstream, async_oneside, reasm, ps_flow_attached, 0);
    return r == PPE_FST_KERNEL ? PPE_FST_KERNEL_ATK : r;
}

// the same with the context's switch for the port-scan detector and sessions on one batch (ppe_flow_stream_portscan;
// csrc/ppe_kernels_flow_portscan_stream.hip, csrc/ppe_kernels_flow_portscan_attack_stream.hip): off, or no table
// flow-attached, ppe_pick_flow_stream_monitors' answer.  On with the detector off (portscan_able != 1, dp_portscan.c:238:
// PortScan_Detect returns at once), the answer as if no table were flow-attached.  On with the detector on: the session
// machine's own conditions first (not attached or tracking off: PLAIN, the detector's planners decide; a configuration
// it is not built for, or a batch past either kernel's workgroup: REFUSE); then the detector kernel with the session
// phase behind it, with the monitors in it only for a context that opted into both pairs (ppe_flow_combine for
// monitors + detector, ppe_flow_stream_monitors for monitors + sessions), else refused as it always was
uint32_t ppe_pick_flow_stream_portscan(uint32_t n, int attached, uint32_t track, uint32_t midstream,
                                       uint32_t async_oneside, uint32_t reasm, int ps_flow_attached,
                                       int atk_flow_attached, uint32_t monitors_on, uint32_t able, uint32_t portscan_on,
                                       uint32_t combine_on) {
    if (portscan_on != 1u || !ps_flow_attached)
        return ppe_pick_flow_stream_monitors(n, attached, track, midstream, async_oneside, reasm, ps_flow_attached,
                                             atk_flow_attached, monitors_on);
    if (able != 1u)
        return ppe_pick_flow_stream_monitors(n, attached, track, midstream, async_oneside, reasm, 0, atk_flow_attached,
                                             monitors_on);
    const uint32_t r = ppe_pick_flow_stream(n, attached, track, midstream, async_oneside, reasm, 0, 0);
    if (r != PPE_FST_KERNEL) return r;
    if (n > PPE_FLOW_PS_MAX) return PPE_FST_REFUSE;
    if (!atk_flow_attached) return PPE_FST_KERNEL_PS;
    return (monitors_on == 1u && combine_on == 1u) ? PPE_FST_KERNEL_PS_ATK : PPE_FST_REFUSE;
}

}  // extern "C"
