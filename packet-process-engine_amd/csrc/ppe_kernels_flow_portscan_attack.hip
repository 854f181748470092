// The one-launch flow kernel with the port-scan detector inside and the attack monitors ahead of it
// (ppe_flow_ps_kernel<MODE, true>: the FLOW + ATK classify body, then the resolve rounds over the packets no monitor
// dropped, then finalize with the syncount_accum count of the SYN-created flows; a table flow-attached with able 1, an
// object flow-attached and ppe_flow_combine on; 1 <= n <= PPE_FLOW_PS_MAX; ppe_pick_flow_combined), as
// a translation unit of its own built from csrc/ppe_kernels.hip, as csrc/ppe_kernels_flow_portscan.hip is
// (ppe_launch_flow_portscan_attack).  Every other kernel is built where it was.
#define PPE_TU_FLOW_PS 2
#include "ppe_kernels.hip"
