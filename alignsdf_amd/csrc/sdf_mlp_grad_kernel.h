// K1G: the fp32 chain (sdf_mlp_kernel.h) in forward mode over a point list - sdf and d sdf / d xyz of every point in one pass.
//
// The Jacobian-vector product of a ReLU network is the same GEMM chain without biases and with the value's ReLU mask, and the
// columns of an MFMA do not interact.  So a point takes a QUAD of B / D columns instead of one:
//   column 4 j      the value: point features (x0, x1, x2), accumulators start from the bias / folded-constants block, ReLU
//   column 4 j + k  tangent d / d x_(k-1), k = 1 .. 3: point features e_(k-1), accumulators start from 0, a row is kept where
//                   the VALUE column's pre-activation of that row is > 0 (torch: the derivative of ReLU at 0 is 0)
// = 8 points per wave, 32 per workgroup.  The tangent lanes read the mask from lane 0 of their quad with a quad permute (DPP): the
// four lanes of a quad lie in the same lane half, so register r holds the same row in all of them.  The kinematic embedding is affine
// in xyz and already folded into the point-feature columns of layers 0 and 2.  Weight stream, LDS ring, constants block, per-sample
// fold and the stage schedule are those of sdf_mlp_body, unchanged.
//
// The value column goes through the operations of sdf_mlp_body<0, 2, false> on the same operands: its sdf is bit-identical to
// asdf_decode_points under ASDF_MATH_F32.  (ReLU there is max(int bits, 0); here every lane selects  bits(quad lane 0) > 0 ? v : +0,
// which for the value lane - its own quad lane 0 - is the same function of every bit pattern.)
// A header of its own, not a template parameter of sdf_mlp_body: every other unit compiles from unchanged text.  The pass of the chain
// itself is sdf_mlp_chain_pass.h, the one text this body, the projection and the tracing body include; with sdf_mlp_body and the forward
// phase of sdf_mlp_vjp_body that makes three texts, and a change to the ring, the waits or the stage schedule is made in those three.
#pragma once
#include "k1_launch.h"
#include "sdf_mlp_kernel.h"

namespace asdf {

constexpr int kGradWavePts = kWavePts / 4;            // 8 points (quads of columns) per wave
constexpr int kGradWgPts = kGradWavePts * kWaves;     // 32 per workgroup

// (GradParams, the extra pointers of this form - a kernel argument of its own beside DecodeParams, as PixelParams is: k1_launch.h)

// quad lane 0's value of v (quad_perm [0, 0, 0, 0]; every lane of a wave is active wherever this is called)
__device__ __forceinline__ int quad0(int v) { return __builtin_amdgcn_mov_dpp(v, 0, 0xf, 0xf, false); }

// value column: ReLU; tangent columns: the value column's mask
__device__ __forceinline__ float relu_quad(float v) { return quad0(__float_as_int(v)) > 0 ? v : 0.0f; }

__device__ __forceinline__ f32x16 relu16q(f32x16 v) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = relu_quad(v[r]);
  return v;
}

// bias block for the value column, 0 for the tangent columns
__device__ __forceinline__ f32x16 load_bias16q(const float* lds_bias, bool tangent) {
  f32x16 v = load_bias16(lds_bias);
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = tangent ? 0.0f : v[r];
  return v;
}

// p.mode == kPointList, affine point features (KP == 2), SeparateDecoder (one output per MLP); p.sdf0 / p.sdf1 and g.grad0 / g.grad1
// may each be null (the host does not evaluate an MLP both of whose outputs are null).
__device__ __forceinline__ void sdf_mlp_grad_body(const DecodeParams& p, const GradParams& g) {
  constexpr int KP = 2;
  using CL = CstLayout<KP>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;
  float* cst = smem + kLdsRingFloats;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int comp = lane & 3;                 // 0 = value, k = tangent d / d x_(k-1)
  const bool tangent = comp != 0;

  const long long npts = p.P;
  const long long ntiles = (npts + kGradWgPts - 1) / kGradWgPts;
  if ((long long)blockIdx.x >= ntiles) return;

  const unsigned lds_ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;

#pragma unroll 1
  for (int slot = 0; slot < p.num_mlps; ++slot) {
    const int head = p.first_mlp + slot;
    const float* hc = cst;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(p.cst + (size_t)head * CL::kFloats);
      for (int i = tid; i < CL::kFloats / 4; i += 256) reinterpret_cast<f32x4*>(cst)[i] = src4[i];
    }
    const float* sbase0 = p.stream + (size_t)head * kStagesHead * kStageFloats;
#pragma unroll
    for (int s = 0; s < kRing - 1; ++s) {
      const float* src = sbase0 + (size_t)s * kStageFloats + wave * 1024 + lane * 4;
      const unsigned dst = lds_ring_base + (s * kStageFloats + wave * 1024) * 4;
#pragma unroll
      for (int c = 0; c < 4; ++c) lds_dma16(src + c * 256, dst + c * 1024);
    }
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");     // my pieces of stage 0 (and my constants loads)
    __syncthreads();                                      // everybody's pieces of stage 0, and the constants
    f32x4 a0 = (reinterpret_cast<const f32x4*>(ring) + lane)[0];
    f32x4 a1 = (reinterpret_cast<const f32x4*>(ring) + lane)[64];

#pragma unroll 1
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const long long pi = tile * kGradWgPts + wave * kGradWavePts + ((lane & 31) >> 2);
      const bool valid = pi < npts;
      float x0 = 0.f, x1 = 0.f, x2 = 0.f;
      if (valid) { x0 = p.xyz[pi * 3 + 0]; x1 = p.xyz[pi * 3 + 1]; x2 = p.xyz[pi * 3 + 2]; }
      // the tangent columns' point is the unit vector of their coordinate
      if (tangent) { x0 = comp == 1 ? 1.0f : 0.0f; x1 = comp == 2 ? 1.0f : 0.0f; x2 = comp == 3 ? 1.0f : 0.0f; }
      // one pass of the chain on the quad: bias block for the value column only, the value column's ReLU mask on all four
#define ASDF_CHAIN_BIAS(P) load_bias16q(P, tangent)
#define ASDF_CHAIN_RELU16(V) relu16q(V)
#define ASDF_CHAIN_RELU(V) relu_quad(V)
#include "sdf_mlp_chain_pass.h"
#undef ASDF_CHAIN_BIAS
#undef ASDF_CHAIN_RELU16
#undef ASDF_CHAIN_RELU
      // value lane: sdf = tanh(s); tangent lane k: grad = (1 - sdf^2) d_k, d_k = its dot without the bias
      const float sdf = tanhf(part + hc[CL::kB4]);
      const float sq = __int_as_float(quad0(__float_as_int(sdf)));
      const float grad = __fmul_rn(__fsub_rn(1.0f, __fmul_rn(sq, sq)), part);
      if (valid && half == 0) {
        float* so = head == 0 ? p.sdf0 : p.sdf1;
        float* go = head == 0 ? g.grad0 : g.grad1;
        if (!tangent) { if (so) so[pi] = sdf; }
        else if (go) go[pi * 3 + (comp - 1)] = grad;
      }
    }   // tiles
  }   // MLPs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace asdf
