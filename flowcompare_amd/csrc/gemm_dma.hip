// The kernels of the LDS-DMA main loop (VAR 9): split-fp16 with A as the limb image its producer wrote.  The loop itself is an inline block
// of the kernel template (gemm_kernel.h says why); gemm.hip describes the variants.
#include "gemm_kernel.h"

namespace fc {

template void launch_cfg<64, 64, 2, 2, EPI_LINEAR, 9>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 9>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_SPLINE, 9>(const GemmParams&, hipStream_t);
template void launch_cfg<64, 64, 2, 1, EPI_AFFINE, 9>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_AFFINE, 9>(const GemmParams&, hipStream_t);

}  // namespace fc
