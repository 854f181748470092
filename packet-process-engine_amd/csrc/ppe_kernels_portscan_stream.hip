// As csrc/ppe_kernels_portscan.hip, with StreamTcp's first-packet verdict as well (STM and PSC both;
// ppe_launch_classify_portscan_stream).
#define PPE_TU_PORTSCAN 2
#include "ppe_kernels.hip"
