// K1T: sphere tracing on the fp32 chain - one ray per MFMA column, free columns refilled from a queue (sdf_mlp_trace_kernel.h).
// SeparateDecoder, affine point features.  A unit of its own, so that every other unit compiles to the same code as without it.
#include "k1_launch.h"
#include "sdf_mlp_trace_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_trace_kernel(const DecodeParams p, const TraceParams q) {
  sdf_mlp_trace_body(p, q);
}

hipError_t k1t_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_trace_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLdsBytes);
}

int k1t_grid(long long rays, int num_cus) {
  const long long fills = (rays + kWgPts - 1) / kWgPts;
  return (int)(fills < num_cus ? fills : num_cus);
}

void k1t_launch(const DecodeParams& p, const TraceParams& q, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_trace_kernel, dim3(grid), dim3(256), kTraceLdsBytes, st, p, q);
}

}  // namespace asdf
