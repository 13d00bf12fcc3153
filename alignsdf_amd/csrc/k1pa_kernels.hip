// K1 on the fp32 MFMA with a pixel-aligned latent (PixelAlign, utils/utils.py:536-566): SeparateDecoder, xyz point features.  The
// fp32 chain of k1_kernels.hip with layer 0 / layer 2 accumulators that start from a bicubic gather of the sample's projected feature
// maps (sdf_mlp_kernel.h: PA) - a unit of its own, so that every other unit compiles to the same code as without it.
#include "k1_launch.h"
#include "sdf_mlp_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_pixel_kernel(const DecodeParams p, const PixelParams px) {
  sdf_mlp_body<0, 2, false, false, true>(p, &px);
}

hipError_t k1pa_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_pixel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
}

void k1pa_launch(const DecodeParams& p, const PixelParams& px, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_pixel_kernel, dim3(grid), dim3(256), kLdsBytes, st, p, px);
}

}  // namespace asdf
