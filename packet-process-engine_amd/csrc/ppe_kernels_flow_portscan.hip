// The one-launch flow kernel with the port-scan detector inside (ppe_flow_ps_kernel: the FLOW classify body, then the
// resolve rounds and finalize with one workgroup, one packet per thread; 1 <= n <= PPE_FLOW_PS_MAX,
// ppe_pick_flow_portscan), as a translation unit of its own built from csrc/ppe_kernels.hip, as
// csrc/ppe_kernels_flow_small.hip is (ppe_launch_flow_portscan).  Every other kernel is built where it was.
#define PPE_TU_FLOW_PS 1
#include "ppe_kernels.hip"
