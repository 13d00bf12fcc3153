// K0's arithmetic as a __device__ body: fold_sample_kernel (fold_kernels.h, one sample into up to three constants images) and
// fold_samples_kernel (k1vb_kernels.hip, the fp32 image of every sample of a batch) are both this text, operation for operation.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_mlp_common.h"

namespace asdf {

// ---------------------------------------------------------------------------------------------
// K0: fold the per-sample constants.  One wave per (head, layer in {0, 2}, output row):
//   c[o]    = b[o] + W_lat[o,:] . latent + W_pt[o,:] . E[:,3]
//   A[o][d] = W_pt[o,:] . E[:,d]            d = 0..2   (column 3 of the K = 4 operand is zero)
// and scatter them into the LDS constants image (sdf_layout.h).
// Reference arithmetic being folded: utils/utils.py:568-569 (latent expand + cat),
// networks/model.py:311-312 (layer-2 skip concat) and utils/utils.py:376-430 (kinematic embedding).
// ---------------------------------------------------------------------------------------------
struct FoldParams {
  const float* wlat;     // [heads][2][512][256]
  const float* wpt;      // [heads][2][512][ASDF_MAX_POINT_FEATS]
  const float* bias02;   // [heads][2][512]
  const float* embed;    // [heads][ASDF_MAX_POINT_FEATS][4]
  const float* latent;   // [256]
  // up to three constants images are folded by ONE launch (blockIdx.y picks the image): the fp32 image, the split-half image and
  // the one-plane image differ in the scales only (they were three launches per sample)
  float* cst[3];         // [heads][cst_offsets(kp).floats]
  int pf[ASDF_MAX_HEADS];
  int kp;                // point-feature K-steps (2 = affine xyz: the A fragments are folded here; > 2 = NeRF: static)
  float s2[3][ASDF_MAX_HEADS];   // scale of the layer-2 constants: 1 for the fp32 image, S_w2 S_x for the split-half image
  float s0[3][ASDF_MAX_HEADS];   // scale of the layer-0 constants: 1, except in the one-plane image (S_x of h0: its accumulators need no rescale)
};

// the rows of workgroup blockIdx.x from (latent, embed) into image `img` of p's scales, whose first head's block is cst_img
__device__ __forceinline__ void fold_sample_body(const FoldParams& p, const float* latent, const float* embed, float* cst_img, int img) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6);   // (head, layer, row)
  const int row = job & (kHidden - 1);
  const int layer = (job >> 9) & 1;
  const int head = job >> 10;
  if (head >= kHeads) return;

  const float* wl = p.wlat + ((size_t)(head * 2 + layer) * kHidden + row) * kLatent;
  float dot = 0.0f;
#pragma unroll
  for (int k = 0; k < kLatent / 64; ++k) dot = fmaf(wl[lane + 64 * k], latent[lane + 64 * k], dot);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);

  const float* wp = p.wpt + ((size_t)(head * 2 + layer) * kHidden + row) * ASDF_MAX_POINT_FEATS;
  const float* E = embed + (size_t)head * ASDF_MAX_POINT_FEATS * 4;
  float a = 0.0f;
  if (lane < 4)
    for (int f = 0; f < p.pf[head]; ++f) a = fmaf(wp[f], E[f * 4 + lane], a);
  const float a3 = __shfl(a, 3);

  const CstOffsets co = cst_offsets(p.kp);
  float* cst = cst_img + (size_t)head * co.floats;
  const int t = row >> 5, rr = row & 31;
  const float sc = layer ? p.s2[img][head] : p.s0[img][head];      // a power of two: the scaled values are exact
  if (lane == 0) {
    const float c = (dot + p.bias02[(head * 2 + layer) * kHidden + row]) + (p.kp == 2 ? a3 : 0.0f);
    const int hh = (rr >> 2) & 1, r = (rr & 3) + 4 * (rr >> 3);
    cst[(layer ? co.c2 : co.c0) + (t * 2 + hh) * 16 + r] = c * sc;
  }
  if (lane < 4 && p.kp == 2) {
    const int step = lane >> 1, hh = lane & 1;
    cst[(layer ? co.a2 : co.a0) + (t * 2 + step) * 64 + hh * 32 + rr] = (lane < 3) ? a * sc : 0.0f;
  }
}

}  // namespace asdf
