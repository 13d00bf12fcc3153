// Launch interface of the fused decoder kernels: each family is its own translation unit (k1_kernels.hip: fp32 MFMA,
// k1_cls_kernels.hip: fp32 MFMA + part classifier, k1h_kernels.hip: split-half fp16 MFMA) and compiles on its own.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_mlp_common.h"

namespace asdf {

// the cluster form of the short-list kernel (sdf_mlp_short_kernel.h)
constexpr int kClusterWgs = 4;                                                 // workgroups per 32-point block in the cluster form
constexpr int kClusterCap = 2048;                                              // longest list the cluster form takes (64 blocks per MLP)
constexpr int kXchgTiles = kTilesL1 + 2 * kTilesHidden;                        // h1 (8 tiles), h2 (16), raw layer-3 accumulators (16)
constexpr int kXchgFloats = kXchgTiles * 64 * 16;                              // 160 KiB per cluster
struct ShortParams {
  float* xchg;          // [clusters][kXchgFloats]
  int* arrivals;        // [clusters][4] (three in use): multiples of 4 between launches
  int cluster_max;      // lists of up to this many points take the cluster form (0 = never)
  int* fault;           // device word (the decoder's status word ASDF_STATUS_CLUSTER_FAULT), sticky: a member waited longer than `timeout_ticks` for another one.
                        // A cluster that sees it writes NO output; the tile form enqueued behind the launch evaluates the list instead
                        // (DecodeParams::short_fault) and the host switches the cluster form off when it reads the word
  unsigned long long timeout_ticks;   // s_memrealtime ticks (100 MHz) a member waits for the others before it gives up
};
constexpr unsigned long long kClusterTimeoutTicks = 100000000ull;              // 1 s: a healthy wait is microseconds

// raise the dynamic-LDS limit of the family's kernels (once per process; cheap)
hipError_t k1_prepare();
hipError_t k1_cls_prepare();
hipError_t k1h_prepare();            // includes the NeRF-encoded family
hipError_t k1h_nerf_prepare();
hipError_t k1s_prepare();           // the one-plane kernels (k1s_kernels.hip)
hipError_t k1s_nerf_prepare();      // the one-plane kernels of the NeRF-encoded decoders (k1s_nerf_kernels.hip)

// kp = point-feature K-steps (2 affine xyz, 5 / 8 NeRF encoding of 9 / 15 features); two_out = CombinedDecoder
void k1_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);
// the fp32 chain over a SHORT voxel list (kGridSubset, kp == 2): one workgroup per 32 points and MLP, output tiles spread over its
// waves - or, for the shortest lists, four workgroups per block (sdf_mlp_short_kernel.h); returns at once for lists longer than p.short_max
void k1_short_launch(bool two_out, const DecodeParams& p, const ShortParams& sp, hipStream_t st);
void k1_cls_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);
// the fp32 chain with a pixel-aligned latent (k1pa_kernels.hip): SeparateDecoder, xyz features, lattice sweeps and point lists
hipError_t k1pa_prepare();
void k1pa_launch(const DecodeParams& p, const PixelParams& px, int grid, hipStream_t st);
// the fp32 chain in forward mode over a point list (k1g_kernels.hip): sdf and d sdf / d xyz; SeparateDecoder, affine point features
struct GradParams {
  float* grad0;         // [P][3] d sdf_hand / d xyz (may be null)
  float* grad1;         // [P][3] d sdf_obj / d xyz (may be null)
};
hipError_t k1g_prepare();
int k1g_grid(long long points, int num_cus);      // workgroups of a launch over `points` points (32 per workgroup tile)
void k1g_launch(const DecodeParams& p, const GradParams& g, int grid, hipStream_t st);
// the fp32 chain in reverse mode over a point list (k1v_kernels.hip, sdf_mlp_vjp_kernel.h): sdf and, for weights dL / d sdf, the gradient
// with respect to the folded per-sample constants, the latent code and the point embedding; SeparateDecoder, affine point features
struct VjpParams {
  const float* streamT; // [heads][kStagesHead][kStageFloats]: W3^T, W2a^T, W1^T as stages (pack_decoder)
  const float* w[2];    // [P] dL / d sdf of the hand / object head; a head is evaluated only when its weights are given
  float* partial;       // [grid][heads][2 (layer 0, layer 2)][512][4]: one block of sums per workgroup
};
hipError_t k1v_prepare();
int k1v_grid(long long points, int num_cus);      // workgroups of a launch over `points` points (128 per workgroup tile)
void k1v_launch(const DecodeParams& p, const VjpParams& v, int grid, hipStream_t st);
// behind it: partial -> d_fold [heads][2][512][4] (heads_mask: bit h = head h was evaluated), then the adjoint of the per-sample fold,
// d_fold -> d_latent [256] / d_embed [heads][max_pf][4] (each may be null)
void k1v_finish(const float* partial, int grid, int heads_mask, float* d_fold, const float* wlat, const float* wpt, int max_pf,
                float* d_latent, float* d_embed, hipStream_t st);
// THE FIT (asdf_fit_codes over B >= 1 samples, asdf_fit_code its B = 1; k1vb_kernels.hip): per step a fold, the LOSS form of the
// kernel above, its finish and an Adam step, every launch carrying all B samples.  In the loss form VjpParams::w holds per-point
// targets (NaN: the point is not in that head's set), the weight is made in the kernel - the clamped-L1 term of fit.fit_sample,
// sdf_mlp_vjp_kernel.h - and the workgroups' fp64 sums of the term go to VjpLossParams::partial.
// Every sample has its own point list, targets, code, embedding, constants block, partial sums and Adam state - sample s runs
// grid_s = k1v_grid(m_s, num_cus) workgroups, workgroup g of it takes tiles g, g + grid_s, ... of its list, and every sum keeps its
// order - so a sample's bits do not depend on its company.  The launch of the loss form has sum_s grid_s workgroups.
struct VjpLossParams {
  float clamp;          // +inf: unclamped
  float inv_n[2];       // 1 / (points of the head's set), rounded once from double: the kernel takes them from its sample's descriptor
  double* partial;      // [sum of grids][heads]
};
// The Adam step on a latent code (one workgroup per sample, a lane per entry), every operation one correctly rounded fp32 operation in
// the order of fit.adam_step_host:
//   g = d_latent + k_prior (z - z0);  m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  z = z - a (m / (sqrt(v) s + eps))
// a sample's state = [z | m | v | d_latent | z0][kLatent]; step = (a, s) of this step; z is also written to z_out (the next fold reads it).
constexpr int kFitStateFloats = 5 * kLatent;
struct AdamRule { float b1, b2, eps, k_prior; };
struct FitSampleDesc {     // device-resident, read-only to the step's kernels
  int first;               // the sample's first point in the concatenated lists
  int m;                   // its points
  int grid;                // its workgroups: k1v_grid(m, num_cus); 0 with heads_mask == 0
  int wg0;                 // its first workgroup in the launch = its first row of the partial sums
  int heads_mask;          // bit h: head h has targets in this sample (0: no data term - d_latent and the history come out as zeros)
  float inv_n[2];          // 1 / (points of the head's set), rounded once from double
  int pad;
  double inv_n_d[2];       // ... and in double, for the history
};
struct FitWg { int sample, g; };      // workgroup of the launch -> (sample, workgroup of the sample)
struct VjpBatchParams {
  const FitSampleDesc* samples;   // [B]
  const FitWg* wgs;               // [sum of grids]
  const float* cst;               // [B][heads][CstLayout<2>::kFloats]: the samples' fp32 constants images
};
constexpr int kFitDescChunk = 16;     // descriptors one k1vb_describe launch carries in its arguments
struct FitDescChunk { int s0, count; FitSampleDesc d[kFitDescChunk]; };
struct FoldParams;
hipError_t k1vb_prepare();
// descriptors and the workgroup map from the host's values, written by a kernel in stream order (no copy, nothing the host must keep)
void k1vb_describe(const FitSampleDesc* host, int B, FitSampleDesc* samples, FitWg* wgs, hipStream_t st);
// the static part of the fp32 constants image into every sample's block (the fold writes the rest)
void k1vb_cst_init(const float* cst_src, float* cst_all, int B, hipStream_t st);
// fold_sample_kernel's arithmetic for image 0 of fp (its scales, weights and point-feature counts), from z [B][256] and
// embed [B][heads][ASDF_MAX_POINT_FEATS][4], into block s of cst_all
void k1vb_fold(const FoldParams& fp, const float* z, const float* embed, float* cst_all, int B, hipStream_t st);
void k1vb_loss_launch(const DecodeParams& p, const VjpParams& v, const VjpLossParams& q, const VjpBatchParams& b, int total_wgs, hipStream_t st);
// per sample: partial -> d_fold[s], d_fold[s] -> d_latent (state[s] + 3 kLatent), and history[s * history_stride] when history is given
void k1vb_finish_loss(const FitSampleDesc* samples, int B, const float* partial, const double* loss_partial, float* d_fold, const float* wlat,
                      const float* wpt, int max_pf, float* state, double* history, long long history_stride, hipStream_t st);
void k1vb_adam_init(float* state, const float* z, const float* z0, int B, hipStream_t st);      // z, z0 [B][256] (z0 null: z)
void k1vb_adam_step(float* state, const float* step, AdamRule rule, float* z_out, int B, hipStream_t st);
// sphere tracing on the fp32 chain (k1t_kernels.hip): one ray per MFMA column, free columns refilled from a per-head queue;
// SeparateDecoder, affine point features.  The rule: sdf_mlp_trace_kernel.h
struct TraceRule {
  int max_steps, refine_steps;
  float step_scale, min_step, max_step;
};
struct TraceOutputs {       // of one head; each may be null
  float* t;                 // [M] (+inf: MISS)
  int* status;              // [M] 0 MISS, 1 HIT, 2 INSIDE, 3 EXHAUSTED
  float* bracket;           // [M][4] (t_lo, t_hi, f_lo, f_hi) of a HIT, zeros otherwise
  int* evals;               // [M] decoder evaluations the ray took
};
struct TraceParams {
  const float* rays;        // [M][8]: o (3), d (3), t0, t1
  long long M;
  TraceRule rule;
  TraceOutputs out[2];      // hand, object
  unsigned long long* queue;   // [2] device words, 0 at launch: the next ray of each head's queue
};
hipError_t k1t_prepare();
int k1t_grid(long long rays, int num_cus);        // workgroups of a launch over `rays` rays (128 columns per workgroup)
void k1t_launch(const DecodeParams& p, const TraceParams& q, int grid, hipStream_t st);
// Newton projection onto one head's zero level on the fp32 chain (k1p_kernels.hip): the gradient form's quad of columns, iterated
// per workgroup tile while a point of it is live; SeparateDecoder, affine point features.  The rule: sdf_mlp_project_kernel.h
struct ProjectRule {
  int max_iters;
  float tol, max_move, min_grad2;
};
struct ProjectParams {      // the input positions are DecodeParams::xyz [P][3], the head DecodeParams::first_mlp; each output may be null
  ProjectRule rule;
  float* xyz_out;           // [P][3] the last iterate
  float* sdf;               // [P] and
  float* grad;              // [P][3] at xyz_out
  float* sdf_in;            // [P] at the input position
  int* status;              // [P] 0 CONVERGED, 1 SPENT, 2 STALLED, 3 BAD
  int* evals;               // [P] decoder evaluations the point took
};
hipError_t k1p_prepare();
int k1p_grid(long long points, int num_cus);      // workgroups of a launch over `points` points (32 per workgroup tile)
void k1p_launch(const DecodeParams& p, const ProjectParams& q, int grid, hipStream_t st);
void k1h_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);
// the W form (16x16x32 MFMAs) of the SeparateDecoder kernels with affine point features: k1hw_kernels.hip
hipError_t k1hw_prepare();
void k1hw_launch(const DecodeParams& p, int grid, hipStream_t st);
void k1hw_subset_launch(const DecodeParams& p, int grid, hipStream_t st);
int k1h_shape();      // 16 = the W form is selected (default), 32 = ASDF_K1H_SHAPE=32 / asdf_set_mfma_shape(32)
int k1h_set_shape(int shape);
void k1h_box_launch(bool two_out, const DecodeParams& p, int grid, hipStream_t st);   // one-plane kernel (k1s_kernels.hip), kp == 2 only; p.stream = high planes
void k1h_subset_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);   // split-half kernel over a voxel list
void k1h_nerf_subset_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);      // ... kp 5 / 8 (k1h_nerf_kernels.hip)
void k1h_nerf_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);      // kp 5 / 8 (k1h_nerf_kernels.hip)
void k1s_nerf_launch(int kp, bool two_out, const DecodeParams& p, int grid, hipStream_t st);      // one-plane kernel, kp 5 / 8; p.stream = high planes

}  // namespace asdf
