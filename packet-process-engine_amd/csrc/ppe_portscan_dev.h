// The port-scan detector's table side, shared by the pre-pass (csrc/ppe_portscan.hip) and the flow-table kernel with the
// detector inside (csrc/ppe_kernels_flow_portscan.hip): the key probe, a record's words, and PortScan_Detec_process.
// Included where the including unit wants the functions to live (the pre-pass: inside its unnamed namespace).
#ifndef PPE_PORTSCAN_DEV_H
#define PPE_PORTSCAN_DEV_H

__device__ __forceinline__ uint32_t ps_hash(uint32_t sip) {  // (any mix: the probe order is not observable)
    uint32_t h = sip * 0x9e3779b1u;
    h ^= h >> 15;
    h *= 0x85ebca6bu;
    return h ^ (h >> 13);
}
__device__ __forceinline__ unsigned long long ps_key(uint32_t sip) { return (1ull << 32) | sip; }
__device__ __forceinline__ uint32_t *ps_rec32(unsigned long long *recs, uint32_t slot) {
    return (uint32_t *)(recs + (size_t)slot * PPE_PS_REC_WORDS);
}
// words of a record as u32: [6] exception [7] last_exception [8] last_dport | flags [9] firstinv
enum { PS_W_EXC = 6, PS_W_LEXC = 7, PS_W_FLAGS = 8, PS_W_FIRST = 9 };

// find the key's slot or claim an empty one (PortScanFind / pcb_insert, :96-118, :225-228).  The table always has
// empty slots (the host rebuilds it before keys could reach 3/4 of the slots)
__device__ __forceinline__ uint32_t ps_find_claim(unsigned long long *keys, uint32_t smask, uint32_t sip, bool &claimed) {
    const unsigned long long key = ps_key(sip);
    uint32_t h = ps_hash(sip) & smask;
    claimed = false;
    for (uint32_t probes = 0; probes <= smask; ++probes, h = (h + 1u) & smask) {
        unsigned long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {
            unsigned long long expect = 0ull;
            if (__hip_atomic_compare_exchange_strong(&keys[h], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                claimed = true;
                return h;
            }
            cur = expect;
        }
        if (cur == key) return h;
    }
    return PPE_PS_NOSLOT;
}

// ---- PortScan_Detec_process (:139-210), verbatim ----
struct PsState {
    uint64_t hold, lc;       // portscan_hold_time, last_cycle
    uint32_t ld, exc, lexc;  // last_dport, exception, last_exception
};
__device__ __forceinline__ PsState ps_load(const unsigned long long *rec) {
    PsState s;
    s.lc = rec[0];
    s.hold = rec[2];
    s.exc = (uint32_t)rec[3];
    s.lexc = (uint32_t)(rec[3] >> 32);
    s.ld = (uint32_t)rec[4] & 0xffffu;
    return s;
}
__device__ __forceinline__ void ps_store(unsigned long long *rec, const PsState &s, uint32_t flags) {
    rec[0] = s.lc;
    rec[2] = s.hold;
    rec[3] = s.exc | ((unsigned long long)s.lexc << 32);
    rec[4] = s.ld | flags;  // (firstinv back to 0)
}
__device__ __forceinline__ uint32_t ps_step(PsState &s, uint32_t d, uint64_t ts, const ppe_ps_kargs &a) {
    if (s.hold) {  // :143-153
        if (ts < s.hold) return PPE_PS_HOLD;
        s.hold = 0;
    }
    if (s.ld == 0u) {  // :155-160 "first create" (a destination port 0 keeps re-arming it)
        s.ld = d;
        s.lc = a.now_cycles;
        return PPE_PS_OK;
    }
    const uint64_t dl = a.now_cycles - s.lc;  // unsigned: now < last_cycle wraps into the last branch
    if (dl < a.rate) {                        // :163-176
        if (s.ld != d) {
            s.ld = d;
            s.exc++;
            if (s.lexc >= a.freq) {
                s.hold = a.now_seconds + a.hold_seconds;
                return PPE_PS_DETECTED;
            }
        }
    } else if (dl > a.rate && dl < 2ull * a.rate) {  // :177-194
        s.lc += a.rate;
        s.lexc = s.exc;
        s.exc = 0;
        if (s.ld != d) {
            s.ld = d;
            s.exc++;
            if (s.lexc >= a.freq) {
                s.hold = a.now_seconds + a.hold_seconds;
                return PPE_PS_DETECTED;
            }
        }
    } else {  // :195-206 (exactly rate, exactly 2 rate, 2 rate and more, wrapped)
        s.lc = a.now_cycles;
        s.lexc = 0;
        s.exc = 0;
        if (s.ld != d) {
            s.ld = d;
            s.exc++;
        }
    }
    return PPE_PS_OK;
}

#endif
