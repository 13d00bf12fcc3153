// K1V: the fp32 chain in reverse mode over point lists - sdf and the gradient of a weighted sum of sdf values with respect to the
// per-sample constants, the latent code and the point embedding (sdf_mlp_vjp_kernel.h).  SeparateDecoder, affine point features.  A
// unit of its own, so that every other unit compiles to the same code as without it.  (The LOSS form of the same body and the fit's
// stream of launches around it: k1vb_kernels.hip.)
#include "k1_launch.h"
#include "sdf_mlp_vjp_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_vjp_kernel(const DecodeParams p, const VjpParams v) {
  sdf_mlp_vjp_body<false>(p, v, VjpLossParams{});
}

__global__ __launch_bounds__(256) void vjp_reduce_kernel(const float* __restrict__ partial, int grid, int heads_mask, float* __restrict__ d_fold) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kVjpFoldFloats) return;
  vjp_reduce_entry(partial, grid, heads_mask, d_fold, e);
}

__global__ __launch_bounds__(256) void vjp_adjoint_kernel(const float* __restrict__ d_fold, const float* __restrict__ wlat,
                                                          const float* __restrict__ wpt, int max_pf, float* __restrict__ d_latent,
                                                          float* __restrict__ d_embed) {
  vjp_adjoint_body(d_fold, wlat, wpt, max_pf, d_latent, d_embed, blockIdx.x);
}

hipError_t k1v_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kVjpLdsBytes);
}

// at most one workgroup per compute unit, persistent over its tiles
int k1v_grid(long long points, int num_cus) {
  const long long ntiles = (points + kWgPts - 1) / kWgPts;
  return (int)(ntiles < num_cus ? ntiles : num_cus);
}

void k1v_launch(const DecodeParams& p, const VjpParams& v, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_vjp_kernel, dim3(grid), dim3(256), kVjpLdsBytes, st, p, v);
}

void k1v_finish(const float* partial, int grid, int heads_mask, float* d_fold, const float* wlat, const float* wpt, int max_pf,
                float* d_latent, float* d_embed, hipStream_t st) {
  hipLaunchKernelGGL(vjp_reduce_kernel, dim3(kVjpFoldFloats / 256), dim3(256), 0, st, partial, grid, heads_mask, d_fold);
  if (d_latent || d_embed)
    hipLaunchKernelGGL(vjp_adjoint_kernel, dim3(kLatent / 4 + kHeads * max_pf), dim3(256), 0, st, d_fold, wlat, wpt, max_pf, d_latent, d_embed);
}

}  // namespace asdf
