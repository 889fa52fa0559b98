// The kernels of the register-staged split main loops: split-fp16 (VAR 5, the default) and split-bf16 (VAR 3).  The loop itself is an inline
// block of the kernel template (gemm_kernel.h says why); gemm.hip describes the variants.
#include "gemm_kernel.h"

namespace fc {

template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_LINEAR, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_LNQ, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_SPLINE, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_SPLINE, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_AFFINE, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_AUGMENT, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 4, 2, EPI_SLICE, 5>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_AFFINE, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_AUGMENT, 3>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_SLICE, 3>(const GemmParams&, hipStream_t);

}  // namespace fc
