// The same kernel with the attack monitors ahead of the detector (ppe_flow_ps_st_kernel with ATK: the FLOW + ATK
// classify body, finalize counting syncount_accum's +1 per SYN-created flow, finish its -1 per completed handshake;
// ppe_flow_stream_portscan with ppe_flow_combine and ppe_flow_stream_monitors): the reference's default
// pipeline in one launch, as a translation unit of its own built from csrc/ppe_kernels.hip the way
// csrc/ppe_kernels_flow_portscan_attack.hip is (ppe_launch_flow_stream_portscan_attack).  Every other kernel is built
// where it was.
#define PPE_TU_FLOW_PS 2
#define PPE_TU_FLOW_PS_ST 1
#include "ppe_kernels.hip"
