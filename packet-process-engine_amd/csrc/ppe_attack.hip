// ppe_attack.hip — the attack monitors' control kernel (dataplane/src/attack/dp_attack.c): the rule load
// (ppe_attack_set), the once-a-second update DP_Attack_Info_Update (ppe_attack_tick, dp_attack.c:712-748) and the clear
// of the drop totals, each a one-workgroup launch ordered on the classify stream (tick and clear fold the classify workgroups' count slots first).  Set and tick end by reducing every
// port's rule and state to its six decision bits (ppe_internal.h PPE_ATK_*): the one word the classify kernels read.
// The monitors themselves are in decode() and the counter flush of csrc/ppe_kernels.hip (ATK).
#include <hip/hip_runtime.h>

#include "ppe_internal.h"

namespace {

__global__ __launch_bounds__(PPE_ATK_CTL_BLOCK) void ppe_attack_ctl_kernel(ppe_atk_kargs a) {
    // tick and clear first fold the classify workgroups' count slots: column j of every slot summed by the block (thread
    // t takes slots t / 16, + 64, ... of column t % 16), the slots zeroed (tick: all of a slot; clear: its totals)
    __shared__ unsigned long long sum[PPE_ATK_SLOT_WORDS];
    if (threadIdx.x < PPE_ATK_SLOT_WORDS) sum[threadIdx.x] = 0;
    __syncthreads();
    if (a.op != PPE_ATK_K_SET) {
        const uint32_t j = threadIdx.x % PPE_ATK_SLOT_WORDS;
        const bool mine = a.op == PPE_ATK_K_TICK || j >= 12u;
        unsigned long long acc = 0;
        for (uint32_t b = threadIdx.x / PPE_ATK_SLOT_WORDS; mine && b < a.nslots; b += PPE_ATK_CTL_BLOCK / PPE_ATK_SLOT_WORDS) {
            unsigned long long *q = &a.slots[(size_t)b * PPE_ATK_SLOT_WORDS + j];
            const unsigned long long v = *q;
            if (v) {
                acc += v;
                *q = 0;
            }
        }
        if (acc) atomicAdd(&sum[j], acc);
    }
    __syncthreads();
    const uint32_t p = threadIdx.x;  // one lane per port from here on
    if (p >= 64u) return;
    uint32_t bits = 0;
    if (p < PPE_ATTACK_PORTS) {
        unsigned long long *s = a.st + PPE_ATK_PORT0 + PPE_ATK_PORT_STRIDE * p;
        if (a.op == PPE_ATK_K_CLEAR) {
            a.st[PPE_ATK_TOTALS + p] = 0;  // land, udpspeed, synspeed, syncount
            return;
        }
        if (a.op == PPE_ATK_K_TICK) {
            s[PPE_ATK_UDP_ACCUM] += sum[3u * p + 0u];
            s[PPE_ATK_SYN_ACCUM] += sum[3u * p + 1u];
            s[PPE_ATK_SYNCNT_ACCUM] += sum[3u * p + 2u];
            a.st[PPE_ATK_TOTALS + p] += sum[12u + p];
        }
        if (a.op == PPE_ATK_K_SET) {
            s[PPE_ATK_RULE_EN] = a.rule[p][0];
            s[PPE_ATK_UDP_SPEED] = a.rule[p][1];
            s[PPE_ATK_SYN_SPEED] = a.rule[p][2];
            s[PPE_ATK_SYN_COUNT] = a.rule[p][3];
        }
        if (a.op == PPE_ATK_K_TICK) {
            s[PPE_ATK_UDPPPS] = s[PPE_ATK_UDP_ACCUM];                // :724-725
            s[PPE_ATK_UDP_ACCUM] = 0;
            if (a.now >= s[PPE_ATK_UDP_HOLD_TIME]) {                 // :727-731 (>=; also taken when nothing is held)
                s[PPE_ATK_UDP_HOLD] = 0;
                s[PPE_ATK_UDP_HOLD_TIME] = 0;
            }
            s[PPE_ATK_SYNPPS] = s[PPE_ATK_SYN_ACCUM];                // :735-736
            s[PPE_ATK_SYN_ACCUM] = 0;
            if (a.now >= s[PPE_ATK_SYN_HOLD_TIME]) {                 // :738-742
                s[PPE_ATK_SYN_HOLD] = 0;
                s[PPE_ATK_SYN_HOLD_TIME] = 0;
            }
            s[PPE_ATK_SYNCNT] = s[PPE_ATK_SYNCNT_ACCUM];             // :744-745
            s[PPE_ATK_SYNCNT_ACCUM] = 0;
        }
        const uint32_t en = (uint32_t)s[PPE_ATK_RULE_EN];
        // uint64 state against the rule's uint32, strictly greater (dp_attack.c:611, :657, :673)
        const bool uh = s[PPE_ATK_UDP_HOLD] != 0, sh = s[PPE_ATK_SYN_HOLD] != 0;
        const bool ud = (en & PPE_ATK_EN_UDP) && (uh || s[PPE_ATK_UDPPPS] > s[PPE_ATK_UDP_SPEED]);
        const bool sd = (en & PPE_ATK_EN_SYN) && (sh || s[PPE_ATK_SYNPPS] > s[PPE_ATK_SYN_SPEED]);
        const bool sc = (en & PPE_ATK_EN_DROP) && s[PPE_ATK_SYNCNT] > s[PPE_ATK_SYN_COUNT];
        bits = ((en & PPE_ATK_EN_LAND) ? PPE_ATK_LAND : 0u) | (ud ? PPE_ATK_UDP_DROP : 0u) |
               ((ud && !uh) ? PPE_ATK_UDP_ARM : 0u) | (sd ? PPE_ATK_SYN_DROP : 0u) | ((sd && !sh) ? PPE_ATK_SYN_ARM : 0u) |
               (sc ? PPE_ATK_SYNCOUNT : 0u);
        bits <<= 6u * p;
    }
    if (a.op == PPE_ATK_K_CLEAR) return;
    bits |= __shfl_xor(bits, 1, 64);
    bits |= __shfl_xor(bits, 2, 64);
    if (p == 0) a.st[PPE_ATK_WORD] = bits;
}

}  // namespace

extern "C" int ppe_launch_attack_ctl(const ppe_atk_kargs *a, void *stream) {
    hipLaunchKernelGGL(ppe_attack_ctl_kernel, dim3(1), dim3(PPE_ATK_CTL_BLOCK), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
