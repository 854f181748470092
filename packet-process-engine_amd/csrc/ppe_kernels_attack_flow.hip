// The flow-table classify kernels with the attack monitors (ppe_classify_kernel<..., FLOW = true, ATK = true>; an object
// attached with ppe_flow_attack_attach) and the post kernel whose finalize counts syncount_accum per created flow
// (ppe_flow_post_kernel<..., ATK = true>), as a translation unit of their own built from csrc/ppe_kernels.hip, as
// csrc/ppe_kernels_attack.hip is (ppe_launch_classify_attack_flow, ppe_launch_flow_post_attack).  Nothing
// flow-attached: the flow-table kernels without the monitors run.
#define PPE_TU_ATTACK_FLOW 1
#include "ppe_kernels.hip"
