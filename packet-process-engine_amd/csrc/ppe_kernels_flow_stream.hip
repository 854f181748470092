// The one-launch flow kernel with the TCP session machine behind the table (ppe_flow_st_kernel: the FLOW classify body,
// finalize with one workgroup, then the session phase and the final verdicts, one packet per thread; 1 <= n <=
// PPE_FLOW_ST_MAX, ppe_pick_flow_stream) and the session records' pass behind a rehash, as a translation
// unit of its own built from csrc/ppe_kernels.hip the way csrc/ppe_kernels_flow_small.hip is (classify_body as a
// function, finalize over LDS the kernel provides; ppe_launch_flow_stream, ppe_launch_flow_stream_rehash).  Every other
// kernel is built where it was.
#define PPE_TU_FLOW_SMALL 3
#define PPE_TU_FLOW_ST 1
#include "ppe_kernels.hip"
