// The stateless classify kernels with StreamTcp's first-packet verdict compiled in (ppe_classify_kernel<..., STM =
// true>, ppe_stream_tcp_set tracking on), built from csrc/ppe_kernels.hip as a translation unit of their own so that
// they compile beside the default kernels, not after them; the default build routes launches with ppe_kargs.stream
// set here (ppe_launch_classify_stream).  With tracking off the default kernels run: no stream code in them.
#define PPE_TU_STREAM 1
#include "ppe_kernels.hip"
