// K1VB: the fit's stream of launches over B >= 1 samples (asdf_fit_codes; asdf_fit_code is B = 1).  The LOSS form of the reverse-mode
// body (sdf_mlp_vjp_kernel.h), where a workgroup first looks up its sample, and per-sample forms of the small kernels around it (fold,
// reduce, adjoint, loss reduce, Adam), each a grid dimension over the samples around the one-sample body.
// A unit of its own, built with k1v_kernels.hip's flags, so that every other unit compiles to the same code as without it.
#include "k1_launch.h"
#include "fold_body.h"
#include "sdf_mlp_vjp_kernel.h"

namespace asdf {

__global__ __launch_bounds__(256, 1) void sdf_mlp_vjp_loss_batch_kernel(const DecodeParams p, const VjpParams v, const VjpLossParams q,
                                                                        const VjpBatchParams b) {
  sdf_mlp_vjp_batch_body(p, v, q, b);
}

hipError_t k1vb_prepare() {
  return hipFuncSetAttribute((const void*)sdf_mlp_vjp_loss_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kVjpLossLdsBytes);
}

void k1vb_loss_launch(const DecodeParams& p, const VjpParams& v, const VjpLossParams& q, const VjpBatchParams& b, int total_wgs, hipStream_t st) {
  hipLaunchKernelGGL(sdf_mlp_vjp_loss_batch_kernel, dim3(total_wgs), dim3(256), kVjpLossLdsBytes, st, p, v, q, b);
}

// one workgroup per descriptor of the chunk: the descriptor itself and the sample's rows of the workgroup map
__global__ __launch_bounds__(256) void fit_describe_kernel(const FitDescChunk c, FitSampleDesc* __restrict__ samples, FitWg* __restrict__ wgs) {
  const int i = blockIdx.x;
  if (i >= c.count) return;
  const FitSampleDesc d = c.d[i];
  if (threadIdx.x == 0) samples[c.s0 + i] = d;
  for (int g = threadIdx.x; g < d.grid; g += 256) wgs[d.wg0 + g] = FitWg{c.s0 + i, g};
}

void k1vb_describe(const FitSampleDesc* host, int B, FitSampleDesc* samples, FitWg* wgs, hipStream_t st) {
  for (int s0 = 0; s0 < B; s0 += kFitDescChunk) {
    FitDescChunk c;
    c.s0 = s0;
    c.count = B - s0 < kFitDescChunk ? B - s0 : kFitDescChunk;
    for (int i = 0; i < kFitDescChunk; ++i) c.d[i] = host[s0 + (i < c.count ? i : 0)];
    hipLaunchKernelGGL(fit_describe_kernel, dim3(c.count), dim3(256), 0, st, c, samples, wgs);
  }
}

constexpr int kCstImageFloats = kHeads * CstLayout<2>::kFloats;

__global__ __launch_bounds__(256) void fit_cst_init_kernel(const float* __restrict__ src, float* __restrict__ cst_all) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kCstImageFloats) cst_all[(size_t)blockIdx.y * kCstImageFloats + i] = src[i];
}

void k1vb_cst_init(const float* cst_src, float* cst_all, int B, hipStream_t st) {
  hipLaunchKernelGGL(fit_cst_init_kernel, dim3((kCstImageFloats + 255) / 256, B), dim3(256), 0, st, cst_src, cst_all);
}

// fold_sample_kernel for image 0, sample blockIdx.y
__global__ __launch_bounds__(256) void fold_samples_kernel(const FoldParams p, const float* __restrict__ z, const float* __restrict__ embed,
                                                           float* __restrict__ cst_all) {
  const size_t s = blockIdx.y;
  fold_sample_body(p, z + s * kLatent, embed + s * (kHeads * ASDF_MAX_POINT_FEATS * 4), cst_all + s * kCstImageFloats, 0);
}

void k1vb_fold(const FoldParams& fp, const float* z, const float* embed, float* cst_all, int B, hipStream_t st) {
  hipLaunchKernelGGL(fold_samples_kernel, dim3(kHeads * 2 * kHidden / 4, B), dim3(256), 0, st, fp, z, embed, cst_all);
}

// vjp_reduce_kernel, sample blockIdx.y: its workgroups' partials in its own workgroup order, under its heads mask
__global__ __launch_bounds__(256) void vjp_reduce_batch_kernel(const FitSampleDesc* __restrict__ samples, const float* __restrict__ partial,
                                                               float* __restrict__ d_fold) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kVjpFoldFloats) return;
  const FitSampleDesc sd = samples[blockIdx.y];
  vjp_reduce_entry(partial + (size_t)sd.wg0 * kVjpFoldFloats, sd.grid, sd.heads_mask, d_fold + (size_t)blockIdx.y * kVjpFoldFloats, e);
}

// vjp_adjoint_kernel's d_latent blocks, sample blockIdx.y: d_fold[s] -> the d_latent row of state[s]
__global__ __launch_bounds__(256) void vjp_adjoint_batch_kernel(const float* __restrict__ d_fold, const float* __restrict__ wlat,
                                                                const float* __restrict__ wpt, int max_pf, float* __restrict__ state) {
  const size_t s = blockIdx.y;
  vjp_adjoint_body(d_fold + s * kVjpFoldFloats, wlat, wpt, max_pf, state + s * kFitStateFloats + 3 * kLatent, nullptr, blockIdx.x);
}

// the data term of one step (vjp_loss_total), sample blockIdx.x: history[s][k]
__global__ void vjp_loss_reduce_batch_kernel(const FitSampleDesc* __restrict__ samples, const double* __restrict__ loss_partial,
                                             double* __restrict__ history, long long history_stride) {
  if (threadIdx.x != 0) return;
  const FitSampleDesc sd = samples[blockIdx.x];
  vjp_loss_total(loss_partial + (size_t)sd.wg0 * kHeads, sd.grid, sd.heads_mask, sd.inv_n_d[0], sd.inv_n_d[1],
                 history + (size_t)blockIdx.x * history_stride);
}

void k1vb_finish_loss(const FitSampleDesc* samples, int B, const float* partial, const double* loss_partial, float* d_fold, const float* wlat,
                      const float* wpt, int max_pf, float* state, double* history, long long history_stride, hipStream_t st) {
  hipLaunchKernelGGL(vjp_reduce_batch_kernel, dim3(kVjpFoldFloats / 256, B), dim3(256), 0, st, samples, partial, d_fold);
  hipLaunchKernelGGL(vjp_adjoint_batch_kernel, dim3(kLatent / 4, B), dim3(256), 0, st, d_fold, wlat, wpt, max_pf, state);
  if (history) hipLaunchKernelGGL(vjp_loss_reduce_batch_kernel, dim3(B), dim3(64), 0, st, samples, loss_partial, history, history_stride);
}

__global__ __launch_bounds__(256) void adam_init_batch_kernel(float* __restrict__ state, const float* __restrict__ z, const float* __restrict__ z0) {
  const size_t s = blockIdx.x;
  adam_init_body(state + s * kFitStateFloats, z + s * kLatent, z0 ? z0 + s * kLatent : nullptr);
}

__global__ __launch_bounds__(256) void adam_step_batch_kernel(float* __restrict__ state, const float* __restrict__ step, const AdamRule r,
                                                              float* __restrict__ z_out) {
  const size_t s = blockIdx.x;
  adam_step_body(state + s * kFitStateFloats, step, r, z_out + s * kLatent);
}

void k1vb_adam_init(float* state, const float* z, const float* z0, int B, hipStream_t st) {
  hipLaunchKernelGGL(adam_init_batch_kernel, dim3(B), dim3(256), 0, st, state, z, z0);
}

void k1vb_adam_step(float* state, const float* step, AdamRule rule, float* z_out, int B, hipStream_t st) {
  hipLaunchKernelGGL(adam_step_batch_kernel, dim3(B), dim3(256), 0, st, state, step, rule, z_out);
}

}  // namespace asdf
