// The one-launch kernel for small fragment batches (ppe_defrag_small_kernel: the six phases of ppe_defrag in one
// workgroup; 1 <= n <= PPE_DEFRAG_SMALL_CUTOFF, ppe_pick_defrag_small), as a translation unit of its own built from
// csrc/ppe_defrag.hip, as csrc/ppe_kernels_flow_small.hip is from csrc/ppe_kernels.hip (ppe_launch_defrag_small).
// Every other kernel is built where it was.
#define PPE_TU_DEFRAG_SMALL 1
#include "ppe_defrag.hip"
