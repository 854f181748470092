// The session and finish phases of the one-launch flow kernels with the TCP session machine behind the table: a fragment
// of a kernel's body, included by the preprocessor where the table is finished (csrc/ppe_kernels.hip: ppe_flow_st_kernel
// and ppe_flow_st_attack_kernel behind flow_finalize_wg; ppe_flow_ps_st_kernel behind the
// detector kernel's finalize phase, §5.17).  Shared as text, not as a function: a __forceinline__ function reordered
// ppe_flow_st_kernel (§5.16), an included fragment leaves every unit the tokens it always compiled.
// It expects in scope: `a` with k (ppe_kargs), t (ppe_flow_small_tail, list pointers NULL), fw_idx, drop_idx, tile_cnt,
// part8, sess, stc; `smem` (the launch's dynamic LDS); the constant ATK; FST_NEW, FST_PORT_SHIFT; and every earlier
// phase's LDS reads finished in program order before this text's first barrier, except in the words the static_asserts
// of the including kernel name.
    // ---- session ----
    // LDS: what the classify phase had in front of the image, free behind the barrier
    using LI = Lds<BLOCK, true, 4u * PPE_UPD_OWNERS * (1u + (PPE_UPD_LDS ? PPE_UPD_CAP : 0u))>;
    // (ATK: est[4] behind g, the establishments of this batch per port; the launch's dynamic LDS is the classify
    // phase's, which these four words do not change)
    static_assert(8u * BLOCK + 4u * (4u * BLOCK + PPE_STC_WORDS + 4u + (ATK ? 4u : 0u)) <= LI::IMGB,
                  "the session arrays fit in front of the image");
    unsigned long long *keys = (unsigned long long *)smem;       // [BLOCK] slot << 32 | index, ~0 for the rest
    uint32_t *pf = smem + 2u * BLOCK, *sq = pf + BLOCK, *ak = sq + BLOCK, *wp = ak + BLOCK;  // by packet index
    uint32_t *sc = wp + BLOCK, *g = sc + PPE_STC_WORDS;          // the stream counters; g[0]: drops, g[1]: lost flows
    const ppe_bdesc &B = a.k.batch[0];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (the counters lie behind finalize's arrays, which its last loop may still be reading in another wave.  The assert
    // below is ppe_flow_st_kernel's layout, flow_finalize_wg's arrays; every including kernel states the disjointness
    // for its own arrays in front of the include: ppe_flow_ps_st_kernel by its two static_asserts there)
    static_assert(PPE_NBINS + 32u + BLOCK + 8u <= 6u * BLOCK, "the counters lie behind finalize's arrays");
    uint32_t *est = g + 4u;  // ATK: SYN_RECV -> ESTABLISHED steps of this batch, by the completing packet's port
    if (tid < PPE_STC_WORDS + 4u + (ATK ? 4u : 0u)) sc[tid] = 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    const uint32_t n = B.n, ntiles = (n + 63u) >> 6, p = tid;
    const bool valid = p < n;
    uint32_t v = valid ? a.t.verdict[p] : 0u;
    bool tracked = valid && (v & 0xffu) == PPE_ST_ACL_FW &&
                   ((v >> 16) & (PPE_F_FLOW | PPE_F_TCP)) == (PPE_F_FLOW | PPE_F_TCP);
    unsigned long long key = ~0ull;
    if (tracked) {
        const uint4 t = ((const uint4 *)B.tuple)[p];
        uint32_t fsip = 0, fports = 0;
        const int32_t s = flow_find(a.k.flow, flow_hashfn_l4(true, t.x, t.y, t.z & 0xffffu, t.z >> 16), t.x, t.y, t.z, 6u,
                                    fsip, fports);
        if (s >= 0) {
            // the TCP header in the window: behind Ethernet, one VLAN tag if decoded, and the IPv4 header (stride >= 144
            // holds every byte read here: at most 18 + 60 + 60)
            const uint8_t *row = B.hdr + (size_t)p * B.stride;
            const uint32_t l3 = 14u + (((t.w >> 8) & 1u) ? 4u : 0u);
            const uint8_t *th = row + l3 + 4u * (row[l3] & 15u);
            const uint32_t wso = PPE_TUPLE_WS(t.w);  // the option's offset from the TCP header, 0: none
            const uint32_t ws = wso ? (uint32_t)th[wso + 2u] : (uint32_t)PPE_SS_NO_WS;
            pf[p] = (uint32_t)th[13] | (((v >> 16) & PPE_F_TOCLIENT) ? 0x100u : 0u) | (ws << 16) |
                    (((v >> 16) & PPE_F_NEWFLOW) ? FST_NEW : 0u);
            if constexpr (ATK)  // m->input_port: the monitors' port byte of this packet (none: port 0)
                if (a.k.fatk_pb) pf[p] |= ((uint32_t)a.k.fatk_pb[p] & 3u) << FST_PORT_SHIFT;
            sq[p] = ((uint32_t)th[4] << 24) | ((uint32_t)th[5] << 16) | ((uint32_t)th[6] << 8) | th[7];
            ak[p] = ((uint32_t)th[8] << 24) | ((uint32_t)th[9] << 16) | ((uint32_t)th[10] << 8) | th[11];
            wp[p] = ((uint32_t)th[14] << 8) | th[15] | ((t.w >> 16) << 16);
            key = ((unsigned long long)(uint32_t)s << 32) | p;
        } else {  // never: a packet with PPE_F_FLOW has a live flow when finalize is done
            tracked = false;
            g[1] = 1u;
        }
    }
    keys[p] = key;
    // bitonic sort of the keys over the batch's power of two (at least one wave)
    uint32_t np2 = 64u;
    while (np2 < n) np2 <<= 1;
    for (uint32_t k = 2u; k <= np2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            __syncthreads();
            const uint32_t q = tid ^ j;
            if (tid < np2 && q > tid) {
                const unsigned long long x = keys[tid], y = keys[q];
                if ((x > y) == ((tid & k) == 0u)) {
                    keys[tid] = y;
                    keys[q] = x;
                }
            }
        }
    }
    __syncthreads();
    // the walk: the first packet of each slot's group
    if (tid < np2) {
        const unsigned long long k0 = keys[tid];
        const uint32_t slot = (uint32_t)(k0 >> 32);
        if (k0 != ~0ull && (tid == 0u || (uint32_t)(keys[tid - 1u] >> 32) != slot)) {
            uint4 *rp = (uint4 *)(a.sess + (size_t)PPE_FLOW_SESS_WORDS * slot);
            uint32_t w[PPE_FLOW_SESS_WORDS];
            {
                const uint4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
                w[0] = r0.x, w[1] = r0.y, w[2] = r0.z, w[3] = r0.w, w[4] = r1.x, w[5] = r1.y, w[6] = r1.z, w[7] = r1.w;
                w[8] = r2.x, w[9] = r2.y, w[10] = r2.z, w[11] = r2.w, w[12] = r3.x, w[13] = r3.y, w[14] = r3.z, w[15] = r3.w;
            }
            PpeSsn x;
            ppe_ss_unpack(w, x);
            uint32_t cport = w[13];  // ATK: flow_item_t.input_port (flow.c:139), the creating packet's port
#pragma unroll 1
            for (uint32_t j = tid; j < np2; ++j) {  // (at most n steps: the group ends where the slot changes)
                const unsigned long long kj = keys[j];
                if ((uint32_t)(kj >> 32) != slot || kj == ~0ull) break;
                const uint32_t i = (uint32_t)kj & (BLOCK - 1u);
                const uint32_t f = pf[i], wl = wp[i];
                if (f & FST_NEW) x = PpeSsn{};  // FlowAdd gave the flow no session yet: the zero record
                if constexpr (ATK)
                    if (f & FST_NEW) cport = (f >> FST_PORT_SHIFT) & 3u;
                const uint32_t before = x.state;
                const PpeSsPkt pk = {f & 0xffu, sq[i], ak[i], wl & 0xffffu, wl >> 16, (f >> 16) & 0xffu, (f >> 8) & 1u};
                sq[i] = ppe_stream_step(x, pk, [&](uint32_t c) { atomicAdd(&sc[c], 1u); });
                // DP_Attack_SynCountFins (stream-tcp.c:608, :660): the step that completes the handshake, on its packet's port
                if constexpr (ATK)
                    if (before == PPE_TCP_SYN_RECV && x.state == PPE_TCP_ESTABLISHED)
                        atomicAdd(&est[(f >> FST_PORT_SHIFT) & 3u], 1u);
            }
            ppe_ss_pack(x, w);
            if constexpr (ATK) w[13] = cport;
            rp[0] = make_uint4(w[0], w[1], w[2], w[3]);
            rp[1] = make_uint4(w[4], w[5], w[6], w[7]);
            rp[2] = make_uint4(w[8], w[9], w[10], w[11]);
            rp[3] = make_uint4(w[12], w[13], w[14], w[15]);
        }
    }
    __syncthreads();
    // ---- finish ----
    const uint32_t reason = tracked ? sq[p] : 0u;
    if (reason) {
        const uint32_t st = reason <= PPE_STC_MIDSTREAM_DISABLE ? reason + 17u : (uint32_t)PPE_ST_STREAM_TRACK_DROP;
        static_assert(PPE_STC_RST_BUT_NO_SESSION + 17u == PPE_ST_STREAM_RST_NO_SESSION &&
                      PPE_STC_MIDSTREAM_DISABLE + 17u == PPE_ST_STREAM_MIDSTREAM_OFF, "StateNone's four reasons");
        const uint32_t fl = (v >> 16) | (st == PPE_ST_STREAM_TRACK_DROP ? reason << PPE_F_STREAM_REASON_SHIFT : 0u);
        v = st | ((uint32_t)PPE_ACT_DROP << 8) | (fl << 16);
        a.t.verdict[p] = v;
    }
    if (wv < ntiles)  // (wave-uniform)
        compact_tile(a.fw_idx, a.drop_idx, a.tile_cnt, n, 0u, wv, lane, valid, (v >> 8) & 0xffu, ~0u, a.part8);
    const uint32_t nd = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(reason != 0u));
    if (lane == 0 && nd) atomicAdd(&g[0], nd);
    __syncthreads();
    if (tid < PPE_STC__COUNT && sc[tid])
        __hip_atomic_fetch_add(&a.stc[tid], (unsigned long long)sc[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 64u && g[0]) {  // output_drop_proc instead of the forward the plain phases counted (flow.c:316-319)
        __hip_atomic_fetch_add(&a.k.cslots[PPE_C_OUT_DROP], (unsigned long long)g[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&a.k.cslots[PPE_C_OUT_FW], 0ull - (unsigned long long)g[0], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 128u && g[1])
        __hip_atomic_fetch_add(&a.k.flow.ctl[PPE_FCTL_ERR], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (ATK)  // syncount_accum -= est[port], modulo 2^64 as the reference's cvmx_atomic_add64 (behind the barrier
                        // above: every walker's LDS adds are in); slot 0 is the slot this workgroup's classify phase flushed into
        if (tid >= 192u && tid < 196u && est[tid - 192u])
            __hip_atomic_fetch_add(&a.k.fatk_slots[3u * (tid - 192u) + 2u], 0ull - (unsigned long long)est[tid - 192u],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
