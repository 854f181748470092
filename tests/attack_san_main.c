/* Stand-alone check of the host-only attack-monitor code under AddressSanitizer and UBSan (tests/test_attack.py builds
 * it with csrc/ppe_stat.c and csrc/launch_plan.cpp, -fsanitize=address,undefined): ppe_format_attack_stat and
 * ppe_format_pkt_stat_atk with exact, tiny and zero capacities, and ppe_pick_attack's table.  Prints the two full
 * texts for the caller to compare with the golden files; any sanitizer report makes the run fail. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ppe_hip.h"

unsigned int ppe_pick_attack(int flow, int attached);
/* csrc/launch_plan.cpp's image planner asks the kernel unit for three constants; nothing here plans an image */
uint32_t ppe_classify_fixed_lds(int block, int pipe, int mode) { (void)block, (void)pipe, (void)mode; return 0; }
uint32_t ppe_flow_lds_extra(void) { return 0; }
uint32_t ppe_flow_waves(void) { return 1; }

static void fill(ppe_attack_info_t *info) {
    memset(info, 0, sizeof *info);
    for (int i = 0; i < PPE_ATTACK_PORTS; i++) {
        uint32_t *pd = (uint32_t *)&info->cfg.pd[i], *td = (uint32_t *)&info->cfg.td[i];
        uint64_t *ai = (uint64_t *)&info->ai[i];
        for (int j = 0; j < 5; j++) pd[j] = 100u * i + j + 1;
        for (int j = 0; j < 11; j++) td[j] = 1000u * i + 7u * j + 3;
        for (int j = 0; j < 14; j++) ai[j] = (1ull << 33) * (j & 1) + 10000ull * i + 13ull * j + 5;
    }
    info->cfg.td[2].syn_count = 0x80000001u;
    info->cfg.hold_seconds = 600;
    info->land_drop = 11;
    info->udpflood_drop = (1ull << 32) + 22;
    info->synflood_drop = 33;
    info->syncount_drop = 44;
}

static int check(int full, const char *ref, int (*fn)(char *, size_t)) {
    const size_t caps[] = {0, 1, 2, 17, (size_t)full, (size_t)full + 1};
    for (size_t k = 0; k < sizeof caps / sizeof caps[0]; k++) {
        char *b = malloc(caps[k] ? caps[k] : 1); /* exactly cap bytes: one byte too many written is a report */
        if (!b || fn(b, caps[k]) != full) return 1;
        if (caps[k] && (strlen(b) != (caps[k] > (size_t)full ? (size_t)full : caps[k] - 1) || strncmp(b, ref, strlen(b))))
            return 1;
        free(b);
    }
    return fn(NULL, 0) != full;
}

static ppe_attack_info_t g_info;
static ppe_counters_t g_cnt;
static ppe_portscan_info_t g_ps;
static int f_stat(char *b, size_t cap) { return ppe_format_attack_stat(&g_info, b, cap); }
static int f_pkt(char *b, size_t cap) { return ppe_format_pkt_stat_atk(&g_cnt, NULL, 0, &g_ps, &g_info, b, cap); }
static int f_pkt0(char *b, size_t cap) { return ppe_format_pkt_stat_atk(&g_cnt, NULL, 0, NULL, NULL, b, cap); }

int main(void) {
    fill(&g_info);
    for (int i = 0; i < 32; i++) g_cnt.c[i] = 1000u + 17u * i;
    g_ps.drop = 987654321;
    const int n1 = f_stat(NULL, 0), n2 = f_pkt(NULL, 0), n3 = f_pkt0(NULL, 0);
    if (n1 <= 0 || n2 <= 0 || n3 <= 0) return 2;
    char *t1 = malloc((size_t)n1 + 1), *t2 = malloc((size_t)n2 + 1), *t3 = malloc((size_t)n3 + 1);
    if (f_stat(t1, (size_t)n1 + 1) != n1 || f_pkt(t2, (size_t)n2 + 1) != n2 || f_pkt0(t3, (size_t)n3 + 1) != n3) return 3;
    if (check(n1, t1, f_stat) || check(n2, t2, f_pkt) || check(n3, t3, f_pkt0)) return 4;
    if (ppe_format_attack_stat(NULL, t1, 1) >= 0 || ppe_format_pkt_stat_atk(NULL, NULL, 0, NULL, NULL, t1, 1) >= 0) return 5;
    if (ppe_pick_attack(0, 1) != 1 || ppe_pick_attack(1, 1) != 0 || ppe_pick_attack(0, 0) != 0 ||
        ppe_pick_attack(1, 0) != 0)
        return 6;
    printf("%s\f%s", t1, t2);
    free(t1);
    free(t2);
    free(t3);
    return 0;
}
