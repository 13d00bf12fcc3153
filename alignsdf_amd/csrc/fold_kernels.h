// Per-sample preparation kernels of the decoder (included by decoder.hip): the fold of the per-sample constants (K0 / K0b), the
// staging of host-resident codes and the pixel-aligned projection.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_mlp_common.h"
#include "fold_body.h"

namespace asdf {

// K0: fold the per-sample constants (fold_body.h: the arithmetic, shared with the batched fold of k1vb_kernels.hip)
__global__ __launch_bounds__(256) void fold_sample_kernel(const FoldParams p) {
  fold_sample_body(p, p.latent, p.embed, p.cst[blockIdx.y], blockIdx.y);
}

// K0b: the point-feature columns and bias rows of layers 0 / 2 of the split-half constants image -> fp16 A operands of the
// one-plane kernels (sdf_layout.h: kA16Floats).  One workgroup per (head, layer), one thread per output row: the largest
// magnitude of the layer's 4 x 512 values picks the power of two T = 2^e (0 <= e <= 15) that brings them under 2^14; every
// value is stored as the two fp16 planes of v / T and the kernel multiplies the point operand by T.  More than 2^29 cannot be
// carried: counted in ASDF_STATUS_RANGE like any other fp16 range violation (the sweep is then refused and repeated as an ordinary one).
__global__ __launch_bounds__(512) void fold_points_f16_kernel(const float* __restrict__ cst_all, float* __restrict__ a16_all, int* status) {
  const int head = blockIdx.x >> 1, layer = blockIdx.x & 1;
  const CstOffsets co = cst_offsets(2);
  const float* cst = cst_all + (size_t)head * co.floats;
  float* a16 = a16_all + (size_t)head * kA16Floats;
  const int row = threadIdx.x, t = row >> 5, rr = row & 31;
  const int abase = layer ? co.a2 : co.a0, cbase = layer ? co.c2 : co.c0;
  float v[4];
  v[0] = cst[abase + (t * 2 + 0) * 64 + 0 * 32 + rr];      // feature d = 2 step + lane half
  v[1] = cst[abase + (t * 2 + 0) * 64 + 1 * 32 + rr];
  v[2] = cst[abase + (t * 2 + 1) * 64 + 0 * 32 + rr];
  v[3] = cst[cbase + (t * 2 + ((rr >> 2) & 1)) * 16 + (rr & 3) + 4 * (rr >> 3)];
  float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
  if (!(m == m)) m = INFINITY;
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
  __shared__ float wmax[8];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  m = wmax[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) m = fmaxf(m, wmax[k]);
  int e = 0;
  if (m > 16384.0f) { int ex; (void)frexpf(m, &ex); e = ex - 14; }       // m in [2^(ex-1), 2^ex): m / 2^e < 2^14
  if (e > 15 || !(m < INFINITY)) { e = 15; if (threadIdx.x == 0 && status) atomicAdd(status + ASDF_STATUS_RANGE, 1); }
  const float T = ldexpf(1.0f, e), inv = ldexpf(1.0f, -e);
  _Float16 hi[4], lo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { const float sv = v[k] * inv; hi[k] = (_Float16)sv; lo[k] = (_Float16)(sv - (float)hi[k]); }
  typedef _Float16 h8v __attribute__((ext_vector_type(8)));
  h8v a, b;
  a[0] = hi[0]; a[1] = hi[1]; a[2] = hi[2]; a[3] = hi[0]; a[4] = hi[1]; a[5] = hi[2]; a[6] = hi[3]; a[7] = lo[3];
  b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = b[4] = b[5] = b[6] = b[7] = (_Float16)0.0f;
  h8v* out = reinterpret_cast<h8v*>(a16 + layer * kA16LayerFloats + t * kA16TileFloats);
  out[rr] = a;              // lane rr:      lane half 0
  out[32 + rr] = b;         // lane 32 + rr: lane half 1
  if (threadIdx.x == 0) a16[2 * kA16LayerFloats + layer] = T;
}

// the per-sample codes of a caller whose codes live on the HOST (pinned, device-addressable memory): one workgroup reads them over
// the link into the decoder's own device words, in stream order, right in front of the fold - no copy engine, no blit kernel, no
// side stream (round 6, VERDICT r05 item 3: the runtime's copy of a 1 KB latent was a shader blit that could not get a wave slot
// while a persistent sweep owned every compute unit and sat resident for the whole sweep - 21.5 ms per sample in the eval-mode trace)
extern "C" __global__ __launch_bounds__(256) void stage_sample_kernel(const float* __restrict__ latent_host, const float* __restrict__ embed_host,
                                                           float* __restrict__ latent_dev, float* __restrict__ embed_dev, int n_embed) {
  const int i = threadIdx.x;
  if (i < kLatent) latent_dev[i] = latent_host[i];
  if (embed_host)
    for (int k = i; k < n_embed; k += 256) embed_dev[k] = embed_host[k];
}

// ---- pixel-aligned latent (PixelAlign, utils/utils.py:536-566) ----------------------------------------------------------------
// channel mean in the reference's order, F.mean(3).mean(2): per channel (one workgroup of 64) the mean of every row over W, then
// the mean of those over H (fp32 sums; the row sums sequential, the row means in a fixed shuffle tree)
extern "C" __global__ __launch_bounds__(64) void channel_mean_kernel(const float* __restrict__ feat, int H, int W, float* __restrict__ mean) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const float* f = feat + (size_t)c * H * W;
  float acc = 0.0f;
  for (int h = lane; h < H; h += 64) {
    float rs = 0.0f;
    for (int w = 0; w < W; ++w) rs = __fadd_rn(rs, f[(size_t)h * W + w]);
    acc = __fadd_rn(acc, __fdiv_rn(rs, (float)W));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, m));
  if (lane == 0) mean[c] = __fdiv_rn(acc, (float)H);
}

// P[head][layer][pixel][512 in [tile][half][r] order] = W_lat(head, layer) [512 x 256] . F [256 x H W]: fp32 FMA chains over the
// 256 channels in order.  64 x 64 output blocks, 256 threads of 4 x 4 outputs, K staged through LDS 16 channels at a time.
extern "C" __global__ __launch_bounds__(256) void pixel_project_kernel(const float* __restrict__ wlat, const float* __restrict__ feat, int HW,
                                                            float* __restrict__ proj) {
  __shared__ float As[16][64 + 4];
  __shared__ float Bs[16][64];
  const int hl = blockIdx.z, row0 = blockIdx.y * 64, pix0 = blockIdx.x * 64;
  const float* Wm = wlat + (size_t)hl * kHidden * kLatent;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  for (int k0 = 0; k0 < kLatent; k0 += 16) {
    for (int e = threadIdx.x; e < 1024; e += 256) {
      const int r = e >> 4, k = e & 15;
      As[k][r] = Wm[(size_t)(row0 + r) * kLatent + k0 + k];
      const int kb = e >> 6, px = e & 63;
      Bs[kb][px] = pix0 + px < HW ? feat[(size_t)(k0 + kb) * HW + pix0 + px] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[k][ty * 4 + i]; b[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = row0 + ty * 4 + i, t = o >> 5, rr = o & 31;
    const int slot = (t * 2 + ((rr >> 2) & 1)) * 16 + (rr & 3) + 4 * (rr >> 3);      // sdf_layout.h: bias arrays [tile][half][r]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pp = pix0 + tx * 4 + j;
      if (pp < HW) proj[((size_t)hl * HW + pp) * kHidden + slot] = acc[i][j];
    }
  }
}

}  // namespace asdf
