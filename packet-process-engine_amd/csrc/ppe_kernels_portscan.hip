// The stateless classify kernels that read the port-scan pre-pass's drop mask (ppe_classify_kernel<..., PSC = true>;
// a table with able = 1 attached, ppe_portscan_attach), without StreamTcp's verdict; built from csrc/ppe_kernels.hip as
// a translation unit of their own, as csrc/ppe_kernels_stream.hip is.  The default build routes launches with
// ppe_kargs.psmask set here (ppe_launch_classify_portscan).  Nothing attached: the default kernels run.
#define PPE_TU_PORTSCAN 1
#include "ppe_kernels.hip"
