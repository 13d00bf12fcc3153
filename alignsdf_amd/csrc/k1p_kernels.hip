// K1P: Newton projection of points onto one head's zero level on the fp32 chain - the gradient form's quad of columns, iterated in
// the kernel while any point of the workgroup's tile is live (sdf_mlp_project_kernel.h).  SeparateDecoder, affine point features.  A
// unit of its own, so that every other unit compiles to the same code as without it.
#include "k1_launch.h"
#include "sdf_mlp_project_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_project_kernel(const DecodeParams p, const ProjectParams q) {
  sdf_mlp_project_body(p, q);
}

hipError_t k1p_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kProjectLdsBytes);
}

int k1p_grid(long long points, int num_cus) {
  const long long ntiles = (points + kGradWgPts - 1) / kGradWgPts;
  return (int)(ntiles < num_cus ? ntiles : num_cus);
}

void k1p_launch(const DecodeParams& p, const ProjectParams& q, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_project_kernel, dim3(grid), dim3(256), kProjectLdsBytes, st, p, q);
}

}  // namespace asdf
