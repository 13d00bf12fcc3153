// K1V: the fp32 chain in reverse mode over point lists - sdf and the gradient of a weighted sum of sdf values with respect to the
// per-sample constants, the latent code and the point embedding (sdf_mlp_vjp_kernel.h).  SeparateDecoder, affine point features.  A
// unit of its own, so that every other unit compiles to the same code as without it.
// Also here: the LOSS form of the same body (weights made in the kernel from per-point targets) and the Adam step that follows it in
// asdf_fit_code's stream of launches.
#include "k1_launch.h"
#include "sdf_mlp_vjp_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_vjp_kernel(const DecodeParams p, const VjpParams v) {
  sdf_mlp_vjp_body<false>(p, v, VjpLossParams{});
}

__global__ __launch_bounds__(256, 1) void sdf_mlp_vjp_loss_kernel(const DecodeParams p, const VjpParams v, const VjpLossParams q) {
  sdf_mlp_vjp_body<true>(p, v, q);
}

hipError_t k1v_prepare() {
  hipError_t e = hipFuncSetAttribute((const void*)sdf_mlp_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kVjpLdsBytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)sdf_mlp_vjp_loss_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kVjpLossLdsBytes);
  return e;
}

// at most one workgroup per compute unit, persistent over its tiles
int k1v_grid(long long points, int num_cus) {
  const long long ntiles = (points + kWgPts - 1) / kWgPts;
  return (int)(ntiles < num_cus ? ntiles : num_cus);
}

void k1v_launch(const DecodeParams& p, const VjpParams& v, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_vjp_kernel, dim3(grid), dim3(256), kVjpLdsBytes, st, p, v);
}

void k1v_loss_launch(const DecodeParams& p, const VjpParams& v, const VjpLossParams& q, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_vjp_loss_kernel, dim3(grid), dim3(256), kVjpLossLdsBytes, st, p, v, q);
}

void k1v_finish(const float* partial, int grid, int heads_mask, float* d_fold, const float* wlat, const float* wpt, int max_pf,
                float* d_latent, float* d_embed, hipStream_t st) {
  hipLaunchKernelGGL(vjp_reduce_kernel, dim3(kVjpFoldFloats / 256), dim3(256), 0, st, partial, grid, heads_mask, d_fold);
  if (d_latent || d_embed)
    hipLaunchKernelGGL(vjp_adjoint_kernel, dim3(kLatent / 4 + kHeads * max_pf), dim3(256), 0, st, d_fold, wlat, wpt, max_pf, d_latent, d_embed);
}

// the data term of one step: per evaluated head the workgroups' fp64 sums in workgroup order, times 1 / n of the head, hand first
__global__ void vjp_loss_reduce_kernel(const double* __restrict__ loss_partial, int grid, int heads_mask, double inv_n0, double inv_n1,
                                       double* __restrict__ history) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  vjp_loss_total(loss_partial, grid, heads_mask, inv_n0, inv_n1, history);
}

void k1v_finish_loss(const float* partial, const double* loss_partial, int grid, int heads_mask, float* d_fold, const float* wlat,
                     const float* wpt, int max_pf, float* d_latent, double inv_n_hand, double inv_n_obj, double* history, hipStream_t st) {
  k1v_finish(partial, grid, heads_mask, d_fold, wlat, wpt, max_pf, d_latent, nullptr, st);
  if (history)
    hipLaunchKernelGGL(vjp_loss_reduce_kernel, dim3(1), dim3(64), 0, st, loss_partial, grid, heads_mask, inv_n_hand, inv_n_obj, history);
}

// (the Adam state's start and step: adam_init_body / adam_step_body of sdf_mlp_vjp_kernel.h, shared with the batched forms)
__global__ __launch_bounds__(256) void adam_init_kernel(float* __restrict__ state, const float* __restrict__ z, const float* __restrict__ z0) {
  adam_init_body(state, z, z0);
}

__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ state, const float* __restrict__ step, const AdamRule r,
                                                        float* __restrict__ z_out) {
  adam_step_body(state, step, r, z_out);
}

void k1v_adam_init(float* state, const float* z, const float* z0, hipStream_t st) {
  hipLaunchKernelGGL(adam_init_kernel, dim3(1), dim3(256), 0, st, state, z, z0);
}

void k1v_adam_step(float* state, const float* step, AdamRule rule, float* z_out, hipStream_t st) {
  hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(256), 0, st, state, step, rule, z_out);
}

}  // namespace asdf
