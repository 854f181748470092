// The one-launch flow kernel with the port-scan detector inside and the TCP session machine behind the table
// (ppe_flow_ps_st_kernel: the detector kernel's classify, setup, resolve and finalize phases, then the session kernel's
// session and finish phases; 1 <= n <= min(PPE_FLOW_PS_MAX, PPE_FLOW_ST_MAX), ppe_pick_flow_stream_portscan; DESIGN.md
// §5.17), as a translation unit of its own built from csrc/ppe_kernels.hip the way csrc/ppe_kernels_flow_portscan.hip is
// (ppe_launch_flow_stream_portscan).  Every other kernel is built where it was.
#define PPE_TU_FLOW_PS 1
#define PPE_TU_FLOW_PS_ST 1
#include "ppe_kernels.hip"
