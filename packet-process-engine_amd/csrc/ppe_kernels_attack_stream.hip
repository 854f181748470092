// The stateless classify kernels with the attack monitors (ppe_classify_kernel<..., ATK = true>; an object attached,
// ppe_attack_attach), as a translation unit of their own built from csrc/ppe_kernels.hip, as csrc/ppe_kernels_stream.hip
// is: PPE_TU_ATTACK 1 the monitors alone, 2 with StreamTcp's verdict, 3 with the port-scan drop mask, 4 with both
// (ppe_launch_classify_attack_stream).  Nothing attached: the kernels without the monitors run.
#define PPE_TU_ATTACK 2
#include "ppe_kernels.hip"
