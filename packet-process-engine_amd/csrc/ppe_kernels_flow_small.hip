// The one-launch kernel for small flow batches (ppe_flow_small_kernel: the FLOW classify body, then finalize with one
// workgroup; 1 <= n <= PPE_FLOW_SMALL_CUTOFF, ppe_pick_flow_small), as a translation unit of its own built from
// csrc/ppe_kernels.hip, as csrc/ppe_kernels_attack_flow.hip is (ppe_launch_flow_small).  Every other kernel is built
// where it was.
#define PPE_TU_FLOW_SMALL 1
#include "ppe_kernels.hip"
