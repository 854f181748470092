// The one-launch kernel for small flow batches with the attack monitors ahead of the table
// (ppe_flow_small_kernel<MODE, true>: the FLOW + ATK classify body, then finalize with one workgroup and the
// syncount_accum count of the SYN-created flows; an object flow-attached and a batch of ppe_classify_flow_host_ports;
// 1 <= n <= PPE_FLOW_SMALL_ATK_CUTOFF; ppe_pick_flow_small_attack), as a translation unit of its own built
// from csrc/ppe_kernels.hip, as csrc/ppe_kernels_flow_portscan_attack.hip is (ppe_launch_flow_small_attack).  Every
// other kernel is built where it was.
#define PPE_TU_FLOW_SMALL 2
#include "ppe_kernels.hip"
