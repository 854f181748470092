// The port-scan detector's pre-pass (PortScan_Detect, dataplane/src/attack/dp_portscan.c:231-272, called on every flow
// miss after syn_check and before the ACL, dataplane/src/flow/flow.c:215-230): stream-ordered ahead of a batch's
// classify launch, it runs the detector for the whole batch with exactly the sequential semantics of one core taking
// the packets in index order, and leaves one 64-bit drop mask per 64-packet tile for the PSC classify kernels
// (csrc/ppe_kernels_portscan.hip).  Built from csrc/ppe_kernels.hip (its decode()), the way ppe_kernels_stream.hip is.
//
//   find      decode each packet; an eligible one (decode's ST_ACL: PPE_F_L4 and not stopped by syn_check) finds or
//             claims its source's slot; a source without a record notes its first appearance (firstinv)
//   creators  per tile, the packets that are their record-less source's first appearance (ballot)
//   scan      exclusive prefix of the tiles' creator counts (one workgroup); free = capacity - live
//   grant     creator of rank r gets a record iff r < free (pcb_create in first-appearance order, :123-137, :254-266)
//   keys      slot << 32 | index for the packets whose source has a record; the others are NOMEM (:257-261)
//   sort      bitonic, 2,048 keys per workgroup in LDS: each source's packets contiguous and in index order
//   heads     per source, its first packet: cycle = now (FCB_UPDATE_TIMESTAMP :109, :263); if no hold is pending and
//             no detection can fire in this batch (last_exception after the first packet's time branch < freq), the
//             first packet runs PortScan_Detec_process here and the source is PARALLEL; otherwise it is queued for
//             the walker
//   members   every later packet of a PARALLEL source, one lane each: after any non-HOLD packet last_dport is that
//             packet's port, and after the first packet every packet is in the `< rate` branch (:163-176) or the
//             first-create branch (:155-160), so packet k is a change iff dport[k-1] != 0 && dport[k] != dport[k-1];
//             one wave-segmented popcount and one atomic per (wave, source) for `exception`.  A scanner owning a
//             quarter of the batch is spread over the whole grid
//   walk      one wave per queued source, 64 members per step: all HOLD when no member's timestamp reaches the hold;
//             a ballot + popcount step when no hold is pending and no detection can fire; a lane-serial step through
//             the verbatim state machine only for the 64-member block where a detection, a hold expiry or the first
//             packet's time branch occurs
//   mask      per tile the ballot of results other than OK (action 0) and the result counts: LDS per workgroup, one
//             global atomic per workgroup and counter
// A batch of at most PPE_PS_SORT_BLOCK packets takes all of these in one launch of one workgroup (ps_fused_kernel,
// below; chosen per batch by ppe_pick_portscan_prepass): a small burst would otherwise queue ten dependent launches
// ahead of a classify launch of a few microseconds.
#define PPE_TU_PORTSCAN_PRE 1
#include <algorithm>

#include "ppe_kernels.hip"

namespace {

constexpr int PS_BLOCK = 256;

#include "ppe_portscan_dev.h"  // ps_hash .. ps_find_claim, PsState, ps_load / ps_store / ps_step

// one workgroup-wide add per counter: lanes add into LDS, thread c < nc flushes counter c
__device__ __forceinline__ void ps_flush(unsigned long long *ctl, const uint32_t *lds, const uint32_t *idx, uint32_t nc) {
    __syncthreads();
    if (threadIdx.x < nc && lds[threadIdx.x])
        __hip_atomic_fetch_add(&ctl[idx[threadIdx.x]], (unsigned long long)lds[threadIdx.x], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// ATK (attack monitors attached as well; chosen on the host): a packet they drop returns before FlowHandlePacket and
// never gets here: the classify kernel's own predicate, from the same decision word and port byte.  Without ATK the
// kernel holds none of it
template <bool ATK>
__global__ __launch_bounds__(PS_BLOCK) void ps_find_kernel(ppe_ps_kargs a) {
    __shared__ uint32_t occ;
    if (threadIdx.x == 0) occ = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PS_BLOCK + threadIdx.x;
    const uint32_t pc = min(i, a.n - 1u);  // clamped: a lane past the end re-reads the last packet
    const uint32_t ro = pc * a.stride;
    const uint4 q0 = gld<uint4>(a.hdr, ro), q1 = gld<uint4>(a.hdr, ro + 16u), q2 = gld<uint4>(a.hdr, ro + 32u);
    const uint32_t w12 = gld<uint32_t>(a.hdr, ro + 48u), wlen = gld<uint32_t>(a.len, 4u * pc);
    const uint32_t w[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, w12};
    uint32_t bits = 0;
    if constexpr (ATK) {
        const uint32_t port = a.atk_ports ? (uint32_t)a.atk_ports[pc] & 3u : 0u;
        bits = (((uint32_t)a.atk_st[PPE_ATK_WORD] >> (6u * port)) & 63u) | (port << 6);
    }
    const Dec k = decode<false, ATK>(w, wlen, a.hdr, pc, a.n, a.stride, a.syn_check, 0u, bits);
    // flow.c:204-215: the packet reaches PortScan_Detect iff it would reach DP_Acl_Lookup
    const bool elig = i < a.n && k.st == ST_ACL;
    uint32_t slot = PPE_PS_NOSLOT;
    if (elig) {
        bool claimed;
        slot = ps_find_claim(a.keys, a.smask, k.sip, claimed);
        if (claimed) atomicAdd(&occ, 1u);
        if (slot != PPE_PS_NOSLOT) {
            uint32_t *r = ps_rec32(a.recs, slot);
            // (read first: once an earlier packet of the source is noted, later ones skip the atomic; a new source
            // owning a quarter of the batch would otherwise queue 260,000 atomics on one word, measured 4.8 ms)
            if (!(__hip_atomic_load(&r[PS_W_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & PPE_PS_LIVE) &&
                __hip_atomic_load(&r[PS_W_FIRST], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ~i)
                __hip_atomic_fetch_max(&r[PS_W_FIRST], ~i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (i < a.n) {
        a.slot_of[i] = slot;
        a.dport[i] = k.dport;
        a.pts[i] = a.ts ? a.ts[i] : a.ts_default;  // mbuf->timestamp
        a.res[i] = slot != PPE_PS_NOSLOT ? (uint8_t)PPE_PS_OK : (uint8_t)PPE_PS_INELIGIBLE;
    }
    const uint32_t idx[1] = {PPE_PSC_OCC};
    ps_flush(a.ctl, &occ, idx, 1u);
}

__device__ __forceinline__ bool ps_is_creator(const ppe_ps_kargs &a, uint32_t i) {
    if (i >= a.n) return false;
    const uint32_t slot = a.slot_of[i];
    if (slot == PPE_PS_NOSLOT) return false;
    const uint32_t *r = ps_rec32(a.recs, slot);
    return !(r[PS_W_FLAGS] & PPE_PS_LIVE) && r[PS_W_FIRST] == ~i;
}

__global__ __launch_bounds__(PS_BLOCK) void ps_creators_kernel(ppe_ps_kargs a) {
    const uint32_t i = blockIdx.x * PS_BLOCK + threadIdx.x;
    const uint64_t m = __builtin_amdgcn_ballot_w64(ps_is_creator(a, i));
    if ((threadIdx.x & 63u) == 0u && (i >> 6) < ((a.n + 63u) >> 6)) {
        a.cmask[i >> 6] = m;
        a.cbase[i >> 6] = (uint32_t)__popcll(m);
    }
}

// one workgroup: cbase[0, tiles) becomes its exclusive prefix; the batch's free count and an empty walker queue
__global__ __launch_bounds__(1024) void ps_scan_kernel(ppe_ps_kargs a) {
    __shared__ uint32_t part[1024];
    const uint32_t tiles = (a.n + 63u) >> 6, t = threadIdx.x;
    const uint32_t per = (tiles + 1023u) / 1024u;
    const uint32_t lo = min(t * per, tiles), hi = min(lo + per, tiles);
    uint32_t sum = 0;
    for (uint32_t j = lo; j < hi; ++j) sum += a.cbase[j];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t c = a.cbase[j];
        a.cbase[j] = run;
        run += c;
    }
    if (t == 0) {
        const unsigned long long live = a.ctl[PPE_PSC_LIVE];
        a.ctl[PPE_PSC_FREE] = live < a.capacity ? a.capacity - live : 0ull;
        a.ctl[PPE_PSC_WORK] = 0ull;
    }
}

__global__ __launch_bounds__(PS_BLOCK) void ps_grant_kernel(ppe_ps_kargs a) {
    __shared__ uint32_t granted;
    if (threadIdx.x == 0) granted = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PS_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    if (ps_is_creator(a, i)) {
        const uint32_t rank = a.cbase[i >> 6] + (uint32_t)__popcll(a.cmask[i >> 6] & ((1ull << lane) - 1ull));
        if ((unsigned long long)rank < a.ctl[PPE_PSC_FREE]) {  // pcb_create: zeroed, sip set (:132-134)
            ps_rec32(a.recs, a.slot_of[i])[PS_W_FLAGS] = PPE_PS_LIVE;
            atomicAdd(&granted, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2u && granted)  // new_pcb (:265) and the live count
        __hip_atomic_fetch_add(&a.ctl[threadIdx.x == 0 ? PPE_PSC_LIVE : PPE_PSC_NEW], (unsigned long long)granted,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(PS_BLOCK) void ps_keys_kernel(ppe_ps_kargs a) {
    const uint32_t i = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (i >= a.npad) return;
    unsigned long long key = ~0ull;
    if (i < a.n) {
        const uint32_t slot = a.slot_of[i];
        if (slot != PPE_PS_NOSLOT) {
            uint32_t *r = ps_rec32(a.recs, slot);
            if (r[PS_W_FLAGS] & PPE_PS_LIVE) {
                key = ((unsigned long long)slot << 32) | i;
            } else {
                a.res[i] = PPE_PS_NOMEM;  // :257-261
                r[PS_W_FIRST] = 0u;       // (every packet of the source writes the same word)
            }
        }
    }
    a.skey[i] = key;
}

// ---- bitonic sort of skey[0, npad) ----
__device__ __forceinline__ void ps_cmpx(unsigned long long &x, unsigned long long &y, bool asc) {
    if ((x > y) == asc) {
        const unsigned long long t = x;
        x = y;
        y = t;
    }
}
// FULL: stages k = 2 .. PPE_PS_SORT_BLOCK of each block; else the passes j = PPE_PS_SORT_BLOCK / 2 .. 1 of stage sort_k
template <bool FULL>
__global__ __launch_bounds__(1024) void ps_sort_lds_kernel(ppe_ps_kargs a) {
    __shared__ unsigned long long s[PPE_PS_SORT_BLOCK];
    const uint32_t base = blockIdx.x * PPE_PS_SORT_BLOCK, t = threadIdx.x;
    s[t] = a.skey[base + t];
    s[t + 1024u] = a.skey[base + t + 1024u];
    __syncthreads();
    for (uint32_t k = FULL ? 2u : a.sort_k; k <= (FULL ? PPE_PS_SORT_BLOCK : a.sort_k); k <<= 1) {
        for (uint32_t j = min(k >> 1, PPE_PS_SORT_BLOCK / 2u); j > 0u; j >>= 1) {
            const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
            ps_cmpx(s[i], s[i | j], ((base + i) & k) == 0u);
            __syncthreads();
        }
    }
    a.skey[base + t] = s[t];
    a.skey[base + t + 1024u] = s[t + 1024u];
}
__global__ __launch_bounds__(PS_BLOCK) void ps_sort_global_kernel(ppe_ps_kargs a) {
    const uint32_t t = blockIdx.x * PS_BLOCK + threadIdx.x, j = a.sort_j;
    if (t >= a.npad / 2u) return;
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
    unsigned long long x = a.skey[i], y = a.skey[i | j];
    const unsigned long long x0 = x;
    ps_cmpx(x, y, (i & a.sort_k) == 0u);
    if (x != x0) {
        a.skey[i] = x;
        a.skey[i | j] = y;
    }
}

__global__ __launch_bounds__(PS_BLOCK) void ps_heads_kernel(ppe_ps_kargs a) {
    const uint32_t j = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (j >= a.npad) return;
    const unsigned long long key = a.skey[j];
    if (key == ~0ull) return;
    const uint32_t slot = (uint32_t)(key >> 32), idx = (uint32_t)key;
    if (j > 0u && (uint32_t)(a.skey[j - 1u] >> 32) == slot) return;
    unsigned long long *rec = a.recs + (size_t)slot * PPE_PS_REC_WORDS;
    rec[1] = a.now_cycles;  // FCB_UPDATE_TIMESTAMP: found (:109) or created (:263), also for packets that come back HOLD
    PsState s = ps_load(rec);
    // last_exception as every later packet of the batch sees it, if no hold is pending
    const uint64_t dl = a.now_cycles - s.lc;
    const uint32_t lexc1 = s.ld == 0u ? s.lexc : dl < a.rate ? s.lexc : (dl > a.rate && dl < 2ull * a.rate) ? s.exc : 0u;
    if (s.hold == 0ull && lexc1 < a.freq) {
        (void)ps_step(s, a.dport[idx], a.pts[idx], a);  // OK: no hold, no detection possible
        ps_store(rec, s, PPE_PS_LIVE);
    } else {
        rec[4] = (uint32_t)rec[4] | PPE_PS_SERIAL;
        const unsigned long long w =
            __hip_atomic_fetch_add(&a.ctl[PPE_PSC_WORK], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.work[w] = j;
    }
}

__global__ __launch_bounds__(PS_BLOCK) void ps_members_kernel(ppe_ps_kargs a) {
    const uint32_t j = blockIdx.x * PS_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    const unsigned long long key = j < a.npad ? a.skey[j] : ~0ull;
    const uint32_t slot = (uint32_t)(key >> 32), idx = (uint32_t)key;
    const unsigned long long prev = (j > 0u && j < a.npad) ? a.skey[j - 1u] : ~0ull;
    const bool valid = key != ~0ull;
    const bool head = valid && (j == 0u || (uint32_t)(prev >> 32) != slot);
    bool par = false;
    uint32_t *r = nullptr;
    if (valid) {
        r = ps_rec32(a.recs, slot);
        par = !(r[PS_W_FLAGS] & PPE_PS_SERIAL);
    }
    bool chg = false;
    if (valid && !head && par) {
        const uint32_t d = a.dport[idx], dp = a.dport[(uint32_t)prev];
        if (dp == 0u) *(unsigned long long *)r = a.now_cycles;  // first create again (:155-160): last_cycle = now
        else chg = d != dp;                                     // :166-170, last_exception < freq: never detected
        const unsigned long long next = j + 1u < a.npad ? a.skey[j + 1u] : ~0ull;
        if ((uint32_t)(next >> 32) != slot || next == ~0ull)    // the source's last packet: its port stays
            r[PS_W_FLAGS] = d | PPE_PS_LIVE;
    }
    // exception += the changes among this wave's packets of the source: the lane that starts a run of one source
    // (the source's head, or lane 0) adds the run's count
    const uint64_t cm = __builtin_amdgcn_ballot_w64(chg);
    const uint64_t sm = __builtin_amdgcn_ballot_w64(head || lane == 0u) | 1ull;
    if ((head || lane == 0u) && valid && par) {
        const uint64_t above = lane == 63u ? 0ull : (sm >> (lane + 1u));
        const uint32_t end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u;  // next run's first lane
        const uint64_t range = (end == 64u ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
        const uint32_t c = (uint32_t)__popcll(cm & range);
        if (c) __hip_atomic_fetch_add(&r[PS_W_EXC], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(PS_BLOCK) void ps_walk_kernel(ppe_ps_kargs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * PS_BLOCK + threadIdx.x) >> 6, nwaves = gridDim.x * (PS_BLOCK / 64);
    const uint32_t nwork = (uint32_t)a.ctl[PPE_PSC_WORK];
    for (uint32_t e = wave; e < nwork; e += nwaves) {
        const uint32_t start = a.work[e];
        const uint32_t slot = (uint32_t)(a.skey[start] >> 32);
        unsigned long long *rec = a.recs + (size_t)slot * PPE_PS_REC_WORDS;
        PsState s = ps_load(rec);  // wave-uniform: every lane carries the same state
        for (uint32_t base = start; base < a.npad; base += 64u) {
            const uint32_t j = base + lane;
            const unsigned long long key = j < a.npad ? a.skey[j] : ~0ull;
            const bool valid = key != ~0ull && (uint32_t)(key >> 32) == slot;
            const uint64_t vm = __builtin_amdgcn_ballot_w64(valid);  // a prefix of the lanes (sorted)
            if (vm == 0ull) break;
            const uint32_t cnt = (uint32_t)__popcll(vm), idx = (uint32_t)key;
            const uint32_t d = valid ? a.dport[idx] : 0u;
            const uint64_t ts = valid ? a.pts[idx] : 0ull;
            uint32_t res = PPE_PS_OK;
            if (s.hold != 0ull && __builtin_amdgcn_ballot_w64(valid && ts >= s.hold) == 0ull) {
                res = PPE_PS_HOLD;  // :145-148 for every member
            } else if (s.hold == 0ull && s.lexc < a.freq && (s.ld == 0u || a.now_cycles - s.lc < a.rate)) {
                // no hold, no detection possible, every member in the first-create or the `< rate` branch
                uint32_t dp = __shfl_up(d, 1);
                if (lane == 0u) dp = s.ld;
                s.exc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid && dp != 0u && d != dp));
                if (__builtin_amdgcn_ballot_w64(valid && dp == 0u)) s.lc = a.now_cycles;
                s.ld = __shfl(d, (int)cnt - 1);
            } else {
                for (uint32_t m = 0; m < cnt; ++m) {
                    const uint32_t dm = __shfl(d, (int)m);
                    const uint32_t tlo = __shfl((uint32_t)ts, (int)m), thi = __shfl((uint32_t)(ts >> 32), (int)m);
                    const uint32_t rm = ps_step(s, dm, ((uint64_t)thi << 32) | tlo, a);
                    if (lane == m) res = rm;
                }
            }
            if (valid) a.res[idx] = (uint8_t)res;
            if (cnt < 64u) break;
        }
        if (lane == 0u) ps_store(rec, s, PPE_PS_LIVE);
    }
}

__global__ __launch_bounds__(PS_BLOCK) void ps_mask_kernel(ppe_ps_kargs a) {
    __shared__ uint32_t cnt[5];
    if (threadIdx.x < 5u) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PS_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t r = i < a.n ? a.res[i] : (uint32_t)PPE_PS_INELIGIBLE;
    // flow.c:216-230: any result but OK, action 0: STAT_ATTACK_PORTSCAN_DROP, return NULL
    const uint64_t dm = __builtin_amdgcn_ballot_w64(r >= PPE_PS_NOMEM && r <= PPE_PS_HOLD && a.action == 0u);
    if (lane == 0u && (i >> 6) < ((a.n + 63u) >> 6)) a.mask[i >> 6] = dm;
    const uint64_t m0 = __builtin_amdgcn_ballot_w64(r == PPE_PS_OK), m1 = __builtin_amdgcn_ballot_w64(r == PPE_PS_NOMEM);
    const uint64_t m2 = __builtin_amdgcn_ballot_w64(r == PPE_PS_DETECTED), m3 = __builtin_amdgcn_ballot_w64(r == PPE_PS_HOLD);
    if (lane < 5u) {
        const uint64_t m = lane == 0u ? m0 : lane == 1u ? m1 : lane == 2u ? m2 : lane == 3u ? m3 : dm;
        if (m) atomicAdd(&cnt[lane], (uint32_t)__popcll(m));
    }
    const uint32_t idx[5] = {PPE_PSC_OK, PPE_PSC_NOMEM, PPE_PSC_DETECTED, PPE_PSC_HOLD, PPE_PSC_DROP};
    ps_flush(a.ctl, cnt, idx, 5u);
}

// ---- the whole pre-pass in one launch, for a batch of at most PPE_PS_SORT_BLOCK packets ----
// One 1,024-thread workgroup runs the phases above one after the other with a workgroup barrier between them; each
// phase is the staged kernel's body over the same batch scratch, so every word it leaves (res, the mask, the records,
// the counters) is the staged launches'.  The sorted keys, the creator masks and prefixes, the walker's queue and the
// counts live in LDS.  Only the power of two L >= n (at least 64) of the keys is sorted: the rest are ~0 and stay last.
// No wait on another workgroup and no unbounded loop: the probe is bounded by the slot mask, the walker by the queue
// length and the sort block.
//
// Memory: the workgroup's waves share one L1, and __syncthreads() orders the plain stores of one phase before the
// plain loads of the next.  An agent-scope atomic is carried out in L2 and does not refresh a line this L1 already
// holds, so a word one phase changes with such an atomic is read afterwards with an agent-scope atomic load (ps_ald):
//   keys        CAS in find; read nowhere else (later phases go by slot_of)
//   firstinv    fetch_max in find; read by creators through ps_ald.  The keys phase (NOMEM) and ps_store / the heads'
//               64-bit store (granted) put it back to 0 with plain stores, as the staged kernels do
//   flags       the same 64-bit word's other half: plain stores only (grant, heads, members, ps_store), but every read
//               of it alone goes through ps_ald as well; ps_load and the heads' SERIAL store read the 64-bit word
//               plainly and keep its low half only, which no atomic writes
//   exception   fetch_add in members, for PARALLEL sources; read again only by later launches (the walker loads the
//               records of SERIAL sources, which members never touches).  ps_load in heads comes before it
//   ctl         PPE_PSC_LIVE is read plainly before this launch adds to it (its last writer is an earlier launch)
__device__ __forceinline__ uint32_t ps_ald(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr uint32_t PSF_BLOCK = 1024;
enum { PSF_OCC = 5, PSF_GRANTED = 6, PSF_WORK = 7, PSF_CNT = 8 };

template <bool ATK>
__global__ __launch_bounds__(PSF_BLOCK) void ps_fused_kernel(ppe_ps_kargs a) {
    __shared__ unsigned long long s[PPE_PS_SORT_BLOCK];
    __shared__ unsigned long long cmask[PPE_PS_SORT_BLOCK / 64u];
    __shared__ uint32_t cbase[PPE_PS_SORT_BLOCK / 64u], work[PPE_PS_SORT_BLOCK];
    __shared__ uint32_t cnt[PSF_CNT];  // [0, 5) the mask phase's counts, then PSF_*
    __shared__ unsigned long long nfree;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t tiles = (a.n + 63u) >> 6, nr = tiles << 6;  // n <= PPE_PS_SORT_BLOCK (ppe_launch_portscan)
    uint32_t L = 64u;
    while (L < a.n) L <<= 1;
    if (t < PSF_CNT) cnt[t] = 0;
    if (t < PPE_PS_SORT_BLOCK / 64u) {
        cmask[t] = 0ull;
        cbase[t] = 0u;
    }
    __syncthreads();

    // find (ps_find_kernel)
    for (uint32_t base = 0; base < nr; base += PSF_BLOCK) {
        const uint32_t i = base + t;
        const uint32_t pc = min(i, a.n - 1u);
        const uint32_t ro = pc * a.stride;
        const uint4 q0 = gld<uint4>(a.hdr, ro), q1 = gld<uint4>(a.hdr, ro + 16u), q2 = gld<uint4>(a.hdr, ro + 32u);
        const uint32_t w12 = gld<uint32_t>(a.hdr, ro + 48u), wlen = gld<uint32_t>(a.len, 4u * pc);
        const uint32_t w[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, w12};
        uint32_t bits = 0;
        if constexpr (ATK) {
            const uint32_t port = a.atk_ports ? (uint32_t)a.atk_ports[pc] & 3u : 0u;
            bits = (((uint32_t)a.atk_st[PPE_ATK_WORD] >> (6u * port)) & 63u) | (port << 6);
        }
        const Dec k = decode<false, ATK>(w, wlen, a.hdr, pc, a.n, a.stride, a.syn_check, 0u, bits);
        const bool elig = i < a.n && k.st == ST_ACL;
        uint32_t slot = PPE_PS_NOSLOT;
        if (elig) {
            bool claimed;
            slot = ps_find_claim(a.keys, a.smask, k.sip, claimed);
            if (claimed) atomicAdd(&cnt[PSF_OCC], 1u);
            if (slot != PPE_PS_NOSLOT) {
                uint32_t *r = ps_rec32(a.recs, slot);
                if (!(ps_ald(&r[PS_W_FLAGS]) & PPE_PS_LIVE) && ps_ald(&r[PS_W_FIRST]) < ~i)
                    __hip_atomic_fetch_max(&r[PS_W_FIRST], ~i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (i < a.n) {
            a.slot_of[i] = slot;
            a.dport[i] = k.dport;
            a.pts[i] = a.ts ? a.ts[i] : a.ts_default;
            a.res[i] = slot != PPE_PS_NOSLOT ? (uint8_t)PPE_PS_OK : (uint8_t)PPE_PS_INELIGIBLE;
        }
    }
    __syncthreads();

    // creators (ps_creators_kernel)
    for (uint32_t base = 0; base < nr; base += PSF_BLOCK) {
        const uint32_t i = base + t;
        bool cr = false;
        if (i < a.n) {
            const uint32_t slot = a.slot_of[i];
            if (slot != PPE_PS_NOSLOT) {
                const uint32_t *r = ps_rec32(a.recs, slot);
                cr = !(ps_ald(&r[PS_W_FLAGS]) & PPE_PS_LIVE) && ps_ald(&r[PS_W_FIRST]) == ~i;
            }
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(cr);
        if (lane == 0u && (i >> 6) < tiles) {
            cmask[i >> 6] = m;
            cbase[i >> 6] = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();

    // scan (ps_scan_kernel): at most 32 tiles
    if (t == 0u) {
        uint32_t run = 0;
        for (uint32_t j = 0; j < tiles; ++j) {
            const uint32_t c = cbase[j];
            cbase[j] = run;
            run += c;
        }
        const unsigned long long live = a.ctl[PPE_PSC_LIVE];
        nfree = live < a.capacity ? a.capacity - live : 0ull;
    }
    __syncthreads();

    // grant (ps_grant_kernel)
    for (uint32_t base = 0; base < nr; base += PSF_BLOCK) {
        const uint32_t i = base + t;
        if (i < a.n && ((cmask[i >> 6] >> lane) & 1ull)) {
            const uint32_t rank = cbase[i >> 6] + (uint32_t)__popcll(cmask[i >> 6] & ((1ull << lane) - 1ull));
            if ((unsigned long long)rank < nfree) {
                ps_rec32(a.recs, a.slot_of[i])[PS_W_FLAGS] = PPE_PS_LIVE;
                atomicAdd(&cnt[PSF_GRANTED], 1u);
            }
        }
    }
    __syncthreads();

    // keys (ps_keys_kernel), into LDS
    for (uint32_t i = t; i < PPE_PS_SORT_BLOCK; i += PSF_BLOCK) {
        unsigned long long key = ~0ull;
        if (i < a.n) {
            const uint32_t slot = a.slot_of[i];
            if (slot != PPE_PS_NOSLOT) {
                uint32_t *r = ps_rec32(a.recs, slot);
                if (ps_ald(&r[PS_W_FLAGS]) & PPE_PS_LIVE) {
                    key = ((unsigned long long)slot << 32) | i;
                } else {
                    a.res[i] = PPE_PS_NOMEM;
                    r[PS_W_FIRST] = 0u;
                }
            }
        }
        s[i] = key;
    }
    __syncthreads();

    // sort (ps_sort_lds_kernel<true> over the first L keys)
    for (uint32_t k = 2u; k <= L; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            if (t < L / 2u) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
                ps_cmpx(s[i], s[i | j], (i & k) == 0u);
            }
            __syncthreads();
        }
    }

    // heads (ps_heads_kernel)
    for (uint32_t j = t; j < L; j += PSF_BLOCK) {
        const unsigned long long key = s[j];
        if (key == ~0ull) continue;
        const uint32_t slot = (uint32_t)(key >> 32), idx = (uint32_t)key;
        if (j > 0u && (uint32_t)(s[j - 1u] >> 32) == slot) continue;
        unsigned long long *rec = a.recs + (size_t)slot * PPE_PS_REC_WORDS;
        rec[1] = a.now_cycles;
        PsState st = ps_load(rec);
        const uint64_t dl = a.now_cycles - st.lc;
        const uint32_t lexc1 =
            st.ld == 0u ? st.lexc : dl < a.rate ? st.lexc : (dl > a.rate && dl < 2ull * a.rate) ? st.exc : 0u;
        if (st.hold == 0ull && lexc1 < a.freq) {
            (void)ps_step(st, a.dport[idx], a.pts[idx], a);
            ps_store(rec, st, PPE_PS_LIVE);
        } else {
            rec[4] = (uint32_t)rec[4] | PPE_PS_SERIAL;
            work[atomicAdd(&cnt[PSF_WORK], 1u)] = j;
        }
    }
    __syncthreads();

    // members (ps_members_kernel): every lane of a wave takes part in the ballots (L is a multiple of 64)
    for (uint32_t base = 0; base < L; base += PSF_BLOCK) {
        const uint32_t j = base + t;
        const unsigned long long key = j < L ? s[j] : ~0ull;
        const uint32_t slot = (uint32_t)(key >> 32), idx = (uint32_t)key;
        const unsigned long long prev = (j > 0u && j < L) ? s[j - 1u] : ~0ull;
        const bool valid = key != ~0ull;
        const bool head = valid && (j == 0u || (uint32_t)(prev >> 32) != slot);
        bool par = false;
        uint32_t *r = nullptr;
        if (valid) {
            r = ps_rec32(a.recs, slot);
            par = !(ps_ald(&r[PS_W_FLAGS]) & PPE_PS_SERIAL);
        }
        bool chg = false;
        if (valid && !head && par) {
            const uint32_t d = a.dport[idx], dp = a.dport[(uint32_t)prev];
            if (dp == 0u) *(unsigned long long *)r = a.now_cycles;
            else chg = d != dp;
            const unsigned long long next = j + 1u < L ? s[j + 1u] : ~0ull;
            if ((uint32_t)(next >> 32) != slot || next == ~0ull) r[PS_W_FLAGS] = d | PPE_PS_LIVE;
        }
        const uint64_t cm = __builtin_amdgcn_ballot_w64(chg);
        const uint64_t sm = __builtin_amdgcn_ballot_w64(head || lane == 0u) | 1ull;
        if ((head || lane == 0u) && valid && par) {
            const uint64_t above = lane == 63u ? 0ull : (sm >> (lane + 1u));
            const uint32_t end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u;
            const uint64_t range = (end == 64u ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
            const uint32_t c = (uint32_t)__popcll(cm & range);
            if (c) __hip_atomic_fetch_add(&r[PS_W_EXC], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();

    // walk (ps_walk_kernel): the workgroup's 16 waves share the queue
    const uint32_t nwork = cnt[PSF_WORK];
    for (uint32_t e = t >> 6; e < nwork; e += PSF_BLOCK / 64u) {
        const uint32_t start = work[e];
        const uint32_t slot = (uint32_t)(s[start] >> 32);
        unsigned long long *rec = a.recs + (size_t)slot * PPE_PS_REC_WORDS;
        PsState st = ps_load(rec);
        for (uint32_t base = start; base < L; base += 64u) {
            const uint32_t j = base + lane;
            const unsigned long long key = j < L ? s[j] : ~0ull;
            const bool valid = key != ~0ull && (uint32_t)(key >> 32) == slot;
            const uint64_t vm = __builtin_amdgcn_ballot_w64(valid);
            if (vm == 0ull) break;
            const uint32_t n = (uint32_t)__popcll(vm), idx = (uint32_t)key;
            const uint32_t d = valid ? a.dport[idx] : 0u;
            const uint64_t ts = valid ? a.pts[idx] : 0ull;
            uint32_t res = PPE_PS_OK;
            if (st.hold != 0ull && __builtin_amdgcn_ballot_w64(valid && ts >= st.hold) == 0ull) {
                res = PPE_PS_HOLD;
            } else if (st.hold == 0ull && st.lexc < a.freq && (st.ld == 0u || a.now_cycles - st.lc < a.rate)) {
                uint32_t dp = __shfl_up(d, 1);
                if (lane == 0u) dp = st.ld;
                st.exc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid && dp != 0u && d != dp));
                if (__builtin_amdgcn_ballot_w64(valid && dp == 0u)) st.lc = a.now_cycles;
                st.ld = __shfl(d, (int)n - 1);
            } else {
                for (uint32_t m = 0; m < n; ++m) {
                    const uint32_t dm = __shfl(d, (int)m);
                    const uint32_t tlo = __shfl((uint32_t)ts, (int)m), thi = __shfl((uint32_t)(ts >> 32), (int)m);
                    const uint32_t rm = ps_step(st, dm, ((uint64_t)thi << 32) | tlo, a);
                    if (lane == m) res = rm;
                }
            }
            if (valid) a.res[idx] = (uint8_t)res;
            if (n < 64u) break;
        }
        if (lane == 0u) ps_store(rec, st, PPE_PS_LIVE);
    }
    __syncthreads();

    // mask (ps_mask_kernel) and the counters
    for (uint32_t base = 0; base < nr; base += PSF_BLOCK) {
        const uint32_t i = base + t;
        const uint32_t r = i < a.n ? a.res[i] : (uint32_t)PPE_PS_INELIGIBLE;
        const uint64_t dm = __builtin_amdgcn_ballot_w64(r >= PPE_PS_NOMEM && r <= PPE_PS_HOLD && a.action == 0u);
        if (lane == 0u && (i >> 6) < tiles) a.mask[i >> 6] = dm;
        const uint64_t m0 = __builtin_amdgcn_ballot_w64(r == PPE_PS_OK), m1 = __builtin_amdgcn_ballot_w64(r == PPE_PS_NOMEM);
        const uint64_t m2 = __builtin_amdgcn_ballot_w64(r == PPE_PS_DETECTED), m3 = __builtin_amdgcn_ballot_w64(r == PPE_PS_HOLD);
        if (lane < 5u) {
            const uint64_t m = lane == 0u ? m0 : lane == 1u ? m1 : lane == 2u ? m2 : lane == 3u ? m3 : dm;
            if (m) atomicAdd(&cnt[lane], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (t < PSF_CNT) {
        // new_pcb (:265) and the live count both take the grants; the walker's queue length stays in the work count
        const uint32_t idx[PSF_CNT] = {PPE_PSC_OK, PPE_PSC_NOMEM, PPE_PSC_DETECTED, PPE_PSC_HOLD,
                                       PPE_PSC_DROP, PPE_PSC_OCC, PPE_PSC_LIVE, PPE_PSC_WORK};
        if (t == PSF_WORK) {
            a.ctl[PPE_PSC_WORK] = cnt[PSF_WORK];
            a.ctl[PPE_PSC_FREE] = nfree;
            if (cnt[PSF_GRANTED])
                __hip_atomic_fetch_add(&a.ctl[PPE_PSC_NEW], (unsigned long long)cnt[PSF_GRANTED], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        } else if (cnt[t]) {
            __hip_atomic_fetch_add(&a.ctl[idx[t]], (unsigned long long)cnt[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// aging (PortScan_timeout, :43-93: now > cycle && now - cycle > FRAG_MAX_TIMEOUT = 20 rate) and slot reclamation: the
// records that stay move into an empty table (dkeys / drecs); keys without a record are dropped
__global__ __launch_bounds__(PS_BLOCK) void ps_rebuild_kernel(ppe_ps_kargs a) {
    __shared__ uint32_t cnt[2];
    if (threadIdx.x < 2u) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (s <= a.smask && a.keys[s] != 0ull) {
        const unsigned long long *rec = a.recs + (size_t)s * PPE_PS_REC_WORDS;
        if ((uint32_t)rec[4] & PPE_PS_LIVE) {
            const uint64_t cyc = rec[1];
            if (a.age && a.now_cycles > cyc && a.now_cycles - cyc > 20ull * a.rate) {  // :70
                atomicAdd(&cnt[0], 1u);
            } else {
                bool claimed;
                const uint32_t sip = (uint32_t)a.keys[s];
                const uint32_t t = ps_find_claim(a.dkeys, a.dmask, sip, claimed);
                unsigned long long *dr = a.drecs + (size_t)t * PPE_PS_REC_WORDS;
                dr[0] = rec[0];
                dr[1] = rec[1];
                dr[2] = rec[2];
                dr[3] = rec[3];
                dr[4] = ((uint32_t)rec[4] & 0xffffu) | PPE_PS_LIVE;
                atomicAdd(&cnt[1], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u && cnt[0]) {  // del_pcb (:76)
        __hip_atomic_fetch_add(&a.ctl[PPE_PSC_DEL], (unsigned long long)cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&a.ctl[PPE_PSC_LIVE], 0ull - cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" int ppe_launch_portscan(int kind, const ppe_ps_kargs *a, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 b(PS_BLOCK);
    const dim3 gn((a->n + PS_BLOCK - 1) / PS_BLOCK), gp((a->npad + PS_BLOCK - 1) / PS_BLOCK);
    switch (kind) {
        case PPE_PS_K_FIND:
            if (a->atk_st) hipLaunchKernelGGL(ps_find_kernel<true>, gn, b, 0, s, *a);
            else hipLaunchKernelGGL(ps_find_kernel<false>, gn, b, 0, s, *a);
            break;
        case PPE_PS_K_CREATORS: hipLaunchKernelGGL(ps_creators_kernel, gn, b, 0, s, *a); break;
        case PPE_PS_K_SCAN: hipLaunchKernelGGL(ps_scan_kernel, dim3(1), dim3(1024), 0, s, *a); break;
        case PPE_PS_K_GRANT: hipLaunchKernelGGL(ps_grant_kernel, gn, b, 0, s, *a); break;
        case PPE_PS_K_KEYS: hipLaunchKernelGGL(ps_keys_kernel, gp, b, 0, s, *a); break;
        case PPE_PS_K_SORT_LDS:
            hipLaunchKernelGGL(ps_sort_lds_kernel<true>, dim3(a->npad / PPE_PS_SORT_BLOCK), dim3(1024), 0, s, *a);
            break;
        case PPE_PS_K_SORT_MERGE_LDS:
            hipLaunchKernelGGL(ps_sort_lds_kernel<false>, dim3(a->npad / PPE_PS_SORT_BLOCK), dim3(1024), 0, s, *a);
            break;
        case PPE_PS_K_SORT_GLOBAL:
            hipLaunchKernelGGL(ps_sort_global_kernel, dim3((a->npad / 2u + PS_BLOCK - 1) / PS_BLOCK), b, 0, s, *a);
            break;
        case PPE_PS_K_HEADS: hipLaunchKernelGGL(ps_heads_kernel, gp, b, 0, s, *a); break;
        case PPE_PS_K_MEMBERS: hipLaunchKernelGGL(ps_members_kernel, gp, b, 0, s, *a); break;
        case PPE_PS_K_WALK: {
            const uint32_t want = (a->n + 63u) / 64u;  // at most one source per packet; 4 waves per workgroup
            hipLaunchKernelGGL(ps_walk_kernel, dim3(std::max(1u, std::min(1024u, (want + 3u) / 4u))), b, 0, s, *a);
            break;
        }
        case PPE_PS_K_MASK: hipLaunchKernelGGL(ps_mask_kernel, gn, b, 0, s, *a); break;
        case PPE_PS_K_FUSED:  // one workgroup: the whole batch fits its sort block
            if (a->n == 0u || a->n > PPE_PS_SORT_BLOCK) return (int)hipErrorInvalidValue;
            if (a->atk_st) hipLaunchKernelGGL(ps_fused_kernel<true>, dim3(1), dim3(PSF_BLOCK), 0, s, *a);
            else hipLaunchKernelGGL(ps_fused_kernel<false>, dim3(1), dim3(PSF_BLOCK), 0, s, *a);
            break;
        case PPE_PS_K_REBUILD:
            hipLaunchKernelGGL(ps_rebuild_kernel, dim3(((size_t)a->smask + PS_BLOCK) / PS_BLOCK), b, 0, s, *a);
            break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
