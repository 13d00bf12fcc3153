// K1P: Newton projection onto the zero level of one head on the fp32 chain - the gradient form's quad of columns
// (sdf_mlp_grad_kernel.h: a point's value and its three tangents under the value's ReLU mask) with the rule below wrapped around the
// tile body.
//
// An iteration is the same 32 points going through the head's weight stream again: to the weight ring that is the next tile (src_of
// wraps as in sdf_mlp_body), and the point a quad feeds may move freely between two passes of the chain.  The four waves of a
// workgroup share the ring and its barriers, so the trip count is WORKGROUP-uniform: a tile is iterated while any of its 32 points is
// live, decided behind a barrier on words in LDS; finished quads ride along frozen (they feed their last position and ignore the
// result).  There is no refill queue: a tile takes max over its points of the evaluations (about 3 at a marching-cubes vertex), and
// the call stays re-entrant.  All eight lanes of a point (its quad in both lane halves) carry the same copy of the point's state: f
// arrives from quad lane 0 and g_k from quad lane k + 1 by quad permutes (DPP), as the ReLU mask travels the other way, and both halves
// see the same bits, so the copies stay equal without talking.
//
// The pass of the chain is sdf_mlp_grad_body's, the same text (sdf_mlp_chain_pass.h with the quad's hooks; itself
// sdf_mlp_body<0, 2, false>'s tile body): a change to the ring, the waits or the stage schedule is made there, in sdf_mlp_body and in
// the forward phase of sdf_mlp_vjp_body.  At every point the kernel evaluates, f is asdf_decode_points' under ASDF_MATH_F32 and g
// asdf_decode_points_grad's, bit for bit.
//
// The rule (all fp32, every operation rounded on its own, no fused multiply-add; per point; ProjectRule below):
//   start     x0 not finite: BAD, 0 evaluations, outputs x0 and zeros.  Else x = x0.
//   evaluate  f, g at x (the first f is sdf_in).
//   decide    |f| <= tol -> CONVERGED; else n2 = (g0 g0 + g1 g1) + g2 g2, !(n2 >= min_grad2) -> STALLED (NaN included); else
//             max_iters steps already taken -> SPENT.
//   step      s = f / n2 (correctly rounded); x_k = clamp(x_k - s g_k, x0_k - max_move, x0_k + max_move), written with comparisons
//             ("v > lo ? v : lo", then "v < hi ? v : hi"); evaluate again.
// The LAST iterate is returned with its f and g.  A point takes at most max_iters + 1 evaluations: the loop is bounded by
// construction, and no workgroup waits for another.
//
// A header of its own, not a template parameter of sdf_mlp_grad_body: every other unit compiles from unchanged text.
#pragma once
#include "k1_launch.h"
#include "sdf_mlp_grad_kernel.h"

namespace asdf {

enum ProjectStatus : int { kProjectConverged = 0, kProjectSpent = 1, kProjectStalled = 2, kProjectBad = 3 };

// the workgroup vote's words live behind the constants block (dynamic LDS: no static LDS shifts the ring's base)
constexpr int kProjectLdsBytes = kLdsBytes + 2 * kWaves * (int)sizeof(int);

__device__ __forceinline__ bool project_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// quad lane K's value of v (quad_perm [K, K, K, K]; every lane of a wave is active wherever this is called)
template <int K>
__device__ __forceinline__ float quad_lane(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xf, 0xf, false));
}

// p.mode == kPointList, affine point features (KP == 2), SeparateDecoder, ONE head (p.first_mlp; p.num_mlps is not read); p.xyz [p.P][3]
// the input positions; every pointer of q may be null.
__device__ __forceinline__ void sdf_mlp_project_body(const DecodeParams& p, const ProjectParams& q) {
  constexpr int KP = 2;
  using CL = CstLayout<KP>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;
  float* cst = smem + kLdsRingFloats;
  int* vote = reinterpret_cast<int*>(cst + CL::kFloats);      // [2][kWaves]: "a point of wave w is live", by vote parity

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int comp = lane & 3;                 // 0 = value, k = tangent d / d x_(k-1)
  const bool tangent = comp != 0;
  const bool writer = half == 0 && !tangent; // one lane of a point's eight writes its outputs

  const long long npts = p.P;
  const long long ntiles = (npts + kGradWgPts - 1) / kGradWgPts;
  if ((long long)blockIdx.x >= ntiles) return;

  const unsigned lds_ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;

  const int head = p.first_mlp;
  const float* hc = cst;
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

  int round = 0;                                        // votes taken so far (never reset: two votes in a row use different words)
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long pi = tile * kGradWgPts + wave * kGradWavePts + ((lane & 31) >> 2);
    const bool valid = pi < npts;
    // ---- this quad's point
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;                // x0: the centre of the trust box
    if (valid) { s0 = p.xyz[pi * 3 + 0]; s1 = p.xyz[pi * 3 + 1]; s2 = p.xyz[pi * 3 + 2]; }
    float c0 = s0, c1 = s1, c2 = s2;                   // x
    int evals = 0;
    bool live = valid;
    if (valid && !(project_finite(s0) && project_finite(s1) && project_finite(s2))) {
      live = false;
      if (writer) {
        if (q.xyz_out) { q.xyz_out[pi * 3 + 0] = s0; q.xyz_out[pi * 3 + 1] = s1; q.xyz_out[pi * 3 + 2] = s2; }
        if (q.sdf) q.sdf[pi] = 0.0f;
        if (q.grad) { q.grad[pi * 3 + 0] = 0.0f; q.grad[pi * 3 + 1] = 0.0f; q.grad[pi * 3 + 2] = 0.0f; }
        if (q.sdf_in) q.sdf_in[pi] = 0.0f;
        if (q.status) q.status[pi] = kProjectBad;
        if (q.evals) q.evals[pi] = 0;
      }
      c0 = c1 = c2 = 0.0f;                              // (it rides along at the origin)
    }

#pragma unroll 1
    for (;; ++round) {
      // ---- the workgroup leaves the tile when every one of its points is done (uniform: the stage barriers below need all four waves
      // on the same trip count).  Two sets of words by parity: a wave that is a vote ahead writes the other set.
      int* votes = vote + (round & 1) * kWaves;
      const int wave_live = __ballot(live) != 0 ? 1 : 0;          // (asked of the whole wave, not under the lane test below)
      if (lane == 0) votes[wave] = wave_live;
      __syncthreads();
      if ((votes[0] | votes[1] | votes[2] | votes[3]) == 0) { ++round; break; }

      float x0 = c0, x1 = c1, x2 = c2;
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
      const float f = quad_lane<0>(sdf);
      const float grad = __fmul_rn(__fsub_rn(1.0f, __fmul_rn(f, f)), part);
      const float g0 = quad_lane<1>(grad), g1 = quad_lane<2>(grad), g2 = quad_lane<3>(grad);

      // ---- the rule (the same on all eight lanes of the point)
      if (live) {
        ++evals;
        if (evals == 1 && writer && q.sdf_in) q.sdf_in[pi] = f;
        const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(g0, g0), __fmul_rn(g1, g1)), __fmul_rn(g2, g2));
        int status = -1;
        if (fabsf(f) <= q.rule.tol) status = kProjectConverged;
        else if (!(n2 >= q.rule.min_grad2)) status = kProjectStalled;
        else if (evals - 1 >= q.rule.max_iters) status = kProjectSpent;
        if (status >= 0) {
          live = false;
          if (writer) {
            if (q.xyz_out) { q.xyz_out[pi * 3 + 0] = c0; q.xyz_out[pi * 3 + 1] = c1; q.xyz_out[pi * 3 + 2] = c2; }
            if (q.sdf) q.sdf[pi] = f;
            if (q.grad) { q.grad[pi * 3 + 0] = g0; q.grad[pi * 3 + 1] = g1; q.grad[pi * 3 + 2] = g2; }
            if (q.status) q.status[pi] = status;
            if (q.evals) q.evals[pi] = evals;
          }
        } else {
          const float s = __fdiv_rn(f, n2);
          const float mm = q.rule.max_move;
          float v, lo, hi;
          v = __fsub_rn(c0, __fmul_rn(s, g0)); lo = __fsub_rn(s0, mm); hi = __fadd_rn(s0, mm);
          v = v > lo ? v : lo; c0 = v < hi ? v : hi;
          v = __fsub_rn(c1, __fmul_rn(s, g1)); lo = __fsub_rn(s1, mm); hi = __fadd_rn(s1, mm);
          v = v > lo ? v : lo; c1 = v < hi ? v : hi;
          v = __fsub_rn(c2, __fmul_rn(s, g2)); lo = __fsub_rn(s2, mm); hi = __fadd_rn(s2, mm);
          v = v > lo ? v : lo; c2 = v < hi ? v : hi;
        }
      }
    }   // iterations
  }   // tiles
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace asdf
