// K1G: the fp32 chain in forward mode over point lists - sdf and its gradient with respect to the query coordinates
// (sdf_mlp_grad_kernel.h).  SeparateDecoder, affine point features.  A unit of its own, so that every other unit compiles to the same
// code as without it.
#include "k1_launch.h"
#include "sdf_mlp_grad_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_grad_kernel(const DecodeParams p, const GradParams g) {
  sdf_mlp_grad_body(p, g);
}

hipError_t k1g_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
}

int k1g_grid(long long points, int num_cus) {
  const long long ntiles = (points + kGradWgPts - 1) / kGradWgPts;
  return (int)(ntiles < num_cus ? ntiles : num_cus);
}

void k1g_launch(const DecodeParams& p, const GradParams& g, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_grad_kernel, dim3(grid), dim3(256), kLdsBytes, st, p, g);
}

}  // namespace asdf
