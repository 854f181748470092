// The one-launch flow kernel with the TCP session machine behind the table and the attack monitors ahead of it
// (ppe_flow_st_attack_kernel: the FLOW + ATK classify body, finalize with one workgroup counting syncount_accum's +1,
// the session phase counting its -1 per completed handshake, the final verdicts; 1 <= n <= PPE_FLOW_ST_MAX,
// ppe_pick_flow_stream_monitors) and the pass ahead of ppe_flow_age's kernel that takes the -1 of every
// flow aged out in its handshake (ppe_flow_st_age_release_kernel), as a translation unit of its own built from
// csrc/ppe_kernels.hip the way csrc/ppe_kernels_flow_stream.hip is (ppe_launch_flow_stream_attack,
// ppe_launch_flow_stream_age_release).  Every other kernel is built where it was.
#define PPE_TU_FLOW_SMALL 3
#define PPE_TU_FLOW_ST 2
#include "ppe_kernels.hip"
