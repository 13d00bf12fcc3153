// K1V: the fp32 chain (sdf_mlp_kernel.h) in REVERSE mode over a point list - sdf of every point and, for caller-supplied weights
// w_p = dL / d sdf_p, the gradient of L with respect to the folded per-sample constants of layers 0 and 2 (sdf_layout.h: A0, c0, A2,
// c2), summed over the list.  Everything per-sample - the latent code, the point embedding - is a linear function of those constants
// (fold_kernels.h), so their gradients follow from this one by the fold's adjoint (vjp_adjoint_kernel below).
//
// The reverse pass of a ReLU network is the same GEMM chain on the transposed weights under the forward pass's masks:
//   u  = w (1 - s^2)
//   d3 = (u w4)      * m3        d2 = (W3^T d3)  * m2        d1 = (W2a^T d2) * m1        d0 = (W1^T d1) * m0
//   d_fold[layer 0][o] = sum_p d0_p[o] (x_p, 1)              d_fold[layer 2][o] = sum_p d2_p[o] (x_p, 1)
// FORWARD PHASE: a copy of sdf_mlp_body<0, 2, false> for a point list (32 points per wave, 128 per workgroup) - the same operations on
// the same operands, so a written sdf is asdf_decode_points' under ASDF_MATH_F32 bit for bit - whose epilogues also keep the masks
// m_l = [pre-activation > 0] as bits: a 32x32 tile is 16 bits per lane, two tiles share a register, m0 .. m3 = 8 + 4 + 8 + 8 = 28.
// (One of the chain's three texts, with sdf_mlp_body and sdf_mlp_chain_pass.h: a change to the ring, the waits or the stage schedule
// is made in all three.  The masks per register and the hoff addresses are why it does not include the pass fragment.)
// REVERSE PHASE: the same stage<> machinery over a second weight image (VjpParams::streamT, packed by pack_decoder with the same
// lambda, indices swapped): W3^T has L3's shape (16 tiles x 4 stages), W2a^T L1's (8 x 4), W1^T L2's (16 x 2), in that order; the ring
// runs on from the forward image into it and wraps back for the next tile (256 stages per tile and head).
//
// REGISTER SCHEME: d3 is never materialised.  Its B operand for K-step s of W3^T is  bit(m3, s) ? u w4[kstep_feature(s, half)] : 0,
// three VALU operations in the shadow of a 64-cycle MFMA, recomputed for each of the 16 output tiles (d3_bop in the body).  Resident
// at the peak (the d1 layer): d2 256 + d1 128 + two accumulators 32 + masks m0, m1 12 + x, keep 7 + the A-fragment window and
// addresses; the forward phase peaks at h1 128 + h2 256 + 32 + masks 28.  d0 is never stored: each tile is reduced as it finishes.
// Compiled with the unit's flags (build_native.TU_FLAGS): 256 + 242 = 498 registers, no scratch, 158 752 B of LDS.  Three things keep
// it there, each marked where it is done: mask bits made without compares and pinned to their tile (relu_bit / relu16m), LDS
// addresses above the 64 KiB an instruction offset reaches rebuilt at their uses (hoff), no branch inside the tile body (reduce_reg).
//
// THE SUMS OVER POINTS: in the D layout a lane is a point, so a d_fold entry is a sum across the 32 lanes of a lane half: a butterfly
// of four DPP steps (xor 1, xor 2, half mirror, mirror inside a row of 16) and one ds_swizzle (xor 16), in a fixed order, after which
// every lane of the half holds the sum (half_sum).  Register r's four sums (d x0, d x1, d x2, d) are kept by the lanes 16 j + r,
// selected by value, and once a tile's 16 registers are in, every lane adds its four sums to its row of a wave-private [2 layers]
// [512][4] LDS block (reduce_flush; lanes l and l + 16 of a half hold the same row and write the same words).  The reduction of tile
// t-1 is spread over the MFMA groups of tile t's first stage (stage_v).  When the workgroup's persistent loop over tiles ends, the
// four waves' blocks are added in wave order into the workgroup's partial, and vjp_reduce_kernel adds the partials in workgroup
// order (fp64 accumulator, fp32 result).  No atomics: two calls on one device and list agree in every bit; a point with w = 0 (and
// every padding column) has u = 0 and adds exact zeros.
// A header of its own, not a template parameter of sdf_mlp_body: every other unit compiles from unchanged text.
#pragma once
#include "k1_launch.h"
#include "sdf_mlp_kernel.h"

namespace asdf {

constexpr int kVjpRowFloats = 4;                                         // (dA[0..2], dc) of one row
constexpr int kVjpHeadFloats = 2 * kHidden * kVjpRowFloats;               // [layer 0 / layer 2][512][4] = 4096
constexpr int kVjpFoldFloats = kHeads * kVjpHeadFloats;                   // d_fold of the C ABI
constexpr int kVjpLdsBytes = kLdsBytes + kWaves * kVjpHeadFloats * 4;     // ring + constants + the waves' sum blocks = 158 752 B
constexpr int kVjpLossLdsBytes = kVjpLdsBytes + kWaves * 8;               // ... + the waves' fp64 loss sums (the loss form)

// (VjpParams, the extra pointers of this form - a kernel argument of its own beside DecodeParams: k1_launch.h)

// 0 or ~0: bit `b` of m (compile-time b)
__device__ __forceinline__ int mask_bit(unsigned m, int b) { return (int)(m << (31 - b)) >> 31; }
__device__ __forceinline__ float keep_if(float v, unsigned m, int b) { return __int_as_float(__float_as_int(v) & mask_bit(m, b)); }

// ReLU of one register as sdf_mlp_body's relu16i does it (integer max on the float bits) and bit `b` of m = [it is > 0]: min(relu, 1) as
// an integer, shifted into place.  The value is made opaque in between: seen through, min(max(x, 0), 1) is rewritten as a compare, and
// the 64-bit lane masks of a layer's compares pile up in scalar registers (1 300 of them spilled).
__device__ __forceinline__ float relu_bit(float x, int b, unsigned& m) {
  int v = max(__float_as_int(x), 0);
  asm("" : "+v"(v));
  m |= (unsigned)min(v, 1) << b;
  return __int_as_float(v);
}
// relu16i of a tile; bits [16 hi, 16 hi + 16) of m = its mask
__device__ __forceinline__ f32x16 relu16m(f32x16 v, int hi, unsigned& m) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = relu_bit(v[r], 16 * hi + r, m);
  // (pinned to this tile: left alone, the 32 terms of a mask register are or-ed where the reverse phase first reads it, and the ReLU
  // values they are made of stay live until then - through scratch)
  asm volatile("" : "+v"(m));
  return v;
}

// a value / pointer that is the same in every lane, held in scalar registers
__device__ __forceinline__ int uniform_i(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ const float* uniform_ptr(const float* q) {
  const unsigned long long a = (unsigned long long)(size_t)q;
  return reinterpret_cast<const float*>((size_t)(((unsigned long long)(unsigned)uniform_i((int)(a >> 32)) << 32) | (unsigned)uniform_i((int)a)));
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// the sum of v over the 32 lanes of the caller's lane half, in every lane of it (every lane of the wave is active): a fixed butterfly
__device__ __forceinline__ float half_sum(float v) {
  v = __fadd_rn(v, dpp_f<0xB1>(v));         // quad_perm [1, 0, 3, 2]
  v = __fadd_rn(v, dpp_f<0x4E>(v));         // quad_perm [2, 3, 0, 1]
  v = __fadd_rn(v, dpp_f<0x141>(v));        // row_half_mirror: the other quad of each 8
  v = __fadd_rn(v, dpp_f<0x140>(v));        // row_mirror: the other 8 of each row of 16
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F)));   // bit mode, xor 16: the other row of the half
  return v;
}

// Register r of d (one masked 32x32 tile of d2 / d0) summed over the points against (x0, x1, x2, 1): lanes 16 j + r of the wave keep the
// four sums in `keep` (selected by value, no branch: the tile body stays one basic block).
__device__ __forceinline__ void reduce_reg(float d, int r, int lane, float x0, float x1, float x2, f32x4& keep) {
  const float s0 = half_sum(__fmul_rn(d, x0)), s1 = half_sum(__fmul_rn(d, x1)), s2 = half_sum(__fmul_rn(d, x2)), s3 = half_sum(d);
  int l15 = lane & 15;
  asm volatile("" : "+v"(l15));             // (one compare per register, made here: sixteen hoisted lane masks would live in scalar registers)
  const bool mine = l15 == r;
  keep[0] = mine ? s0 : keep[0];
  keep[1] = mine ? s1 : keep[1];
  keep[2] = mine ? s2 : keep[2];
  keep[3] = mine ? s3 : keep[3];
}
// ... and, once the 16 registers of tile t are in: row 32 t + tile_row(lane & 15, half) of this wave's sum block += keep.  Lanes l and
// l + 16 of a half hold the same row and the same sums: they read, add and write the same words.
__device__ __forceinline__ void reduce_flush(const f32x4& keep, int t, int lane_row, float* rows) {
  asm volatile("" : "+v"(lane_row));        // (the address is made here: hoisted, the 32 row addresses of a lane live across the tile loop)
  f32x4* p = reinterpret_cast<f32x4*>(rows + (32 * t + lane_row) * kVjpRowFloats);
  const f32x4 a = *p;
  *p = f32x4{__fadd_rn(a[0], keep[0]), __fadd_rn(a[1], keep[1]), __fadd_rn(a[2], keep[2]), __fadd_rn(a[3], keep[3])};
}

// stage<KT, Q, SLOT, 0> (sdf_mlp_kernel.h) for the reverse layers - the same ring, waits, barrier and DMA pieces - with two openings:
// the B operand of K-step s is bop(s, grp(g)) (grp: once per group of four K-steps), and epi(g) is issued behind EVERY group, so that
// an epilogue as long as a tile's reduction spreads over the stage's MFMAs; a scheduling barrier per group keeps it there.
template <int Q, int SLOT, class Grp, class Bop, class Epi>
__device__ __forceinline__ void stage_v(f32x16& acc, Grp&& grp, Bop&& bop, const float* ring, const float* next_src, unsigned lds_ring_base,
                                         int lane, int wave, f32x4& a0, f32x4& a1, Epi&& epi) {
  constexpr int nslot = (SLOT + kRing - 1) % kRing;
  const float* src = next_src + wave * 1024 + lane * 4;
  const unsigned dst = lds_ring_base + (nslot * kStageFloats + wave * 1024) * 4;
  const f32x4* cur = reinterpret_cast<const f32x4*>(ring + SLOT * kStageFloats) + lane;
  const f32x4* nxt = reinterpret_cast<const f32x4*>(ring + ((SLOT + 1) % kRing) * kStageFloats) + lane;
  f32x4 abuf[18];
  abuf[0] = a0;
  abuf[1] = a1;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    if (g == 8) {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    abuf[g + 2] = g + 2 < 16 ? cur[(g + 2) * 64] : nxt[(g + 2 - 16) * 64];
    const f32x4 gv = grp(g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc = ASDF_MFMA(abuf[g][j], bop(Q * 64 + g * 4 + j, gv), acc);
      if (g == 8) {
        if (j == 0) lds_dma16_off<0>(src, dst);
        else if (j == 1) lds_dma16_off<1024>(src, dst);
        else if (j == 2) lds_dma16_off<2048>(src, dst);
        else lds_dma16_off<3072>(src, dst);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    epi(g);
    __builtin_amdgcn_sched_barrier(0);
  }
  a0 = abuf[16];
  a1 = abuf[17];
}

// acc (raw reverse accumulators of tile t) under the forward mask of the same rows
__device__ __forceinline__ f32x16 mask_tile(const f32x16& acc, unsigned m, int hi) {
  f32x16 d;
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = keep_if(acc[r], m, 16 * hi + r);
  return d;
}

// The sum of a double over the 32 lanes of the caller's lane half, in every lane of it: the butterfly of half_sum on 64-bit values
// (loss form only; the terms are fp32 values, so the fp64 sum of a list is exact far beyond any list length)
__device__ __forceinline__ double half_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m <= 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// p.mode == kPointList, affine point features (KP == 2), SeparateDecoder; p.sdf0 / p.sdf1 may be null.  The host evaluates a head only
// when its weights v.w[head] are given.
// LOSS (the fit form, k1vb_kernels.hip): v.w[head] holds per-point TARGETS t instead of weights, and the weight is formed where the
// value f is: with c = q.clamp,  r = clip(f, -c, c) - clip(t, -c, c),  l = |r|,  w = (t is NaN or f < -c or f > c) ? 0 : sign(r) q.inv_n[head]
// - the clamped-L1 term of fit.fit_sample and its autograd weight (sign(0) = 0, the clamp's mask inclusive as torch.clamp's backward).
// A NaN target takes the point out of the head's set (l = 0, w = 0).  The l of a workgroup's points are added in fp64 (per tile: the
// half's butterfly, then the wave's LDS word; the waves in wave order) into q.partial[workgroup][head].  Everything behind w is the
// reverse phase of the weight form, the same text.
// Its launch carries the point lists of B >= 1 samples.  The body depends on its launch only through the workgroup's index and the
// launch's size, p.P / xyz / cst / first_mlp / num_mlps, v.w[] / partial and q.inv_n[] / partial; sdf_mlp_vjp_batch_body below makes
// those for the workgroup's sample and hands in its index inside the sample (sample_wg) and the sample's own grid (sample_nwg) -
// everything behind this line is then the one-list form, the same text.
template <bool LOSS>
__device__ __forceinline__ void sdf_mlp_vjp_body(const DecodeParams& p, const VjpParams& v, const VjpLossParams& q, unsigned sample_wg = 0,
                                                 unsigned sample_nwg = 0) {
  // (read where they are used, as the weight form always has: made once up here, the launch's size lives across the tile loop)
  auto wg = [&]() -> unsigned { if constexpr (LOSS) return sample_wg; else return blockIdx.x; };
  auto nwg = [&]() -> unsigned { if constexpr (LOSS) return sample_nwg; else return gridDim.x; };
  constexpr int KP = 2;
  using CL = CstLayout<KP>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;
  float* cst = smem + kLdsRingFloats;
  float* sums = cst + CL::kFloats;                       // [wave][layer 0 / 2][512][4]
  double* lsum = reinterpret_cast<double*>(sums + kWaves * kVjpHeadFloats);      // [wave] (LOSS only: kVjpLossLdsBytes)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  float* mysums = sums + wave * kVjpHeadFloats;

  const long long npts = p.P;
  const long long ntiles = (npts + kWgPts - 1) / kWgPts;
  if ((long long)wg() >= ntiles) return;                 // (never: k1v_grid launches at most one workgroup per tile)

  const unsigned lds_ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;

#pragma unroll 1
  for (int slot = 0; slot < p.num_mlps; ++slot) {
    const int head = p.first_mlp + slot;
    const float* hc = cst;
    const float* wgt;
    if constexpr (LOSS) wgt = head ? v.w[1] : v.w[0];      // (v and q are the workgroup's own copies there: no indexed reads of them)
    else wgt = v.w[head];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(p.cst + (size_t)head * CL::kFloats);
      for (int i = tid; i < CL::kFloats / 4; i += 256) reinterpret_cast<f32x4*>(cst)[i] = src4[i];
      for (int i = tid; i < kWaves * kVjpHeadFloats / 4; i += 256) reinterpret_cast<f32x4*>(sums)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (LOSS) { if (tid < kWaves) lsum[tid] = 0.0; }
    }
    const float* fwd0 = p.stream + (size_t)head * kStagesHead * kStageFloats;
    const float* rev0 = v.streamT + (size_t)head * kStagesHead * kStageFloats;
#pragma unroll
    for (int s = 0; s < kRing - 1; ++s) {
      const float* src = fwd0 + (size_t)s * kStageFloats + wave * 1024 + lane * 4;
      const unsigned dst = lds_ring_base + (s * kStageFloats + wave * 1024) * 4;
#pragma unroll
      for (int c = 0; c < 4; ++c) lds_dma16(src + c * 256, dst + c * 1024);
    }
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");     // my pieces of stage 0 (and my constants loads)
    __syncthreads();                                      // everybody's pieces of stage 0, the constants, the cleared sums
    f32x4 a0 = (reinterpret_cast<const f32x4*>(ring) + lane)[0];
    f32x4 a1 = (reinterpret_cast<const f32x4*>(ring) + lane)[64];

#pragma unroll 1
    for (long long tile = wg(); tile < ntiles; tile += nwg()) {
      const long long pi = tile * kWgPts + wave * kWavePts + (lane & 31);
      const bool valid = pi < npts;
      float x0 = 0.f, x1 = 0.f, x2 = 0.f, wp = 0.f;
      if (valid) {
        x0 = p.xyz[pi * 3 + 0]; x1 = p.xyz[pi * 3 + 1]; x2 = p.xyz[pi * 3 + 2];
        if constexpr (!LOSS) wp = wgt[pi];                      // (the loss form reads its target where it is used)
      }
      float bp[KP];
      bp[0] = half ? x1 : x0;
      bp[1] = half ? 0.0f : x2;
      // stage s of this tile: [0, 128) the forward image, [128, 256) the transposed one, then the forward image again (the next tile);
      // the bases are made opaque per tile so that the per-lane source addresses are not hoisted out of the tile loop (spills)
      const float* fbase = fwd0;
      const float* rbase = rev0;
      if constexpr (LOSS) {      // (derived from descriptor words: named uniform where the constraint below needs a scalar)
        fbase = uniform_ptr(fbase);
        rbase = uniform_ptr(rbase);
      }
      asm volatile("" : "+s"(fbase));
      asm volatile("" : "+s"(rbase));
      auto src_of = [&](int s) -> const float* {   // s = stage index within the tile + 3
        return s < kStagesHead ? fbase + (size_t)s * kStageFloats
                               : (s < 2 * kStagesHead ? rbase + (size_t)(s - kStagesHead) * kStageFloats
                                                      : fbase + (size_t)(s - 2 * kStagesHead) * kStageFloats);
      };
      // 16 half, made wherever it is used: the LDS addresses built on it (one per tile and array: the constants block lies above the
      // 64 KiB an instruction offset reaches) are loop-invariant and would otherwise be hoisted out of the tile loop - ~50 registers
      auto hoff = [&]() { int hv = half * 16; asm volatile("" : "+v"(hv)); return hv; };
      unsigned m0[kTilesHidden / 2], m1[kTilesL1 / 2], m2[kTilesHidden / 2], m3[kTilesHidden / 2];
#pragma unroll
      for (int i = 0; i < kTilesHidden / 2; ++i) m0[i] = m2[i] = m3[i] = 0u;
#pragma unroll
      for (int i = 0; i < kTilesL1 / 2; ++i) m1[i] = 0u;

#define ASDF_STAGE(KT, Q, SLOT, ACC, HIN, SIDX, EPI) \
  stage<KT, Q, SLOT, 0>(ACC, HIN, ring, src_of((SIDX) + 3), lds_ring_base, lane, wave, a0, a1, EPI)

      float u;
      {
        // ================= forward phase (sdf_mlp_body<0, 2, false>, masks kept) =================
        f32x16 h0[kTilesHidden];
#pragma unroll
        for (int t = 0; t < kTilesHidden; ++t) {
          f32x16 acc = load_bias16(hc + CL::kC0 + t * 32 + hoff());
#pragma unroll
          for (int s = 0; s < KP; ++s) acc = ASDF_MFMA(hc[CL::kA0 + (t * KP + s) * 64 + lane], bp[s], acc);
          h0[t] = relu16m(acc, t & 1, m0[t >> 1]);
        }

        // ---- layer 1: 512 -> 256
        f32x16 h1[kTilesL1];
        f32x16 acc1[2];
#pragma unroll
        for (int t = 0; t < kTilesL1; ++t) {
          f32x16& acc = acc1[t & 1];
          acc = load_bias16(hc + CL::kB1 + t * 32 + hoff());
          auto epi = [&]() {
            if (t == 0) return;
            h1[t - 1] = relu16m(acc1[(t - 1) & 1], (t - 1) & 1, m1[(t - 1) >> 1]);
          };
          ASDF_STAGE(16, 0, 0, acc, h0, t * 4 + 0, epi);
          ASDF_STAGE(16, 1, 1, acc, h0, t * 4 + 1, NoEpilogue());
          ASDF_STAGE(16, 2, 2, acc, h0, t * 4 + 2, NoEpilogue());
          ASDF_STAGE(16, 3, 3, acc, h0, t * 4 + 3, NoEpilogue());
        }

        // ---- layer 2: [h1 (256) | xyz (4)] -> 512
        f32x16 h2[kTilesHidden];
        f32x16 acc2[2];
#pragma unroll
        for (int t = 0; t < kTilesHidden; ++t) {
          f32x16& acc = acc2[t & 1];
          acc = load_bias16(hc + CL::kC2 + t * 32 + hoff());
#pragma unroll
          for (int s = 0; s < KP; ++s) acc = ASDF_MFMA(hc[CL::kA2 + (t * KP + s) * 64 + lane], bp[s], acc);
          auto epi = [&]() {
            if (t > 0) {
              h2[t - 1] = relu16m(acc2[(t - 1) & 1], (t - 1) & 1, m2[(t - 1) >> 1]);
            } else {
              h1[kTilesL1 - 1] = relu16m(acc1[(kTilesL1 - 1) & 1], (kTilesL1 - 1) & 1, m1[(kTilesL1 - 1) >> 1]);
            }
          };
          constexpr int S0 = kStagesL1;
          if (t & 1) {
            ASDF_STAGE(8, 0, 2, acc, h1, S0 + t * 2 + 0, epi);
            ASDF_STAGE(8, 1, 3, acc, h1, S0 + t * 2 + 1, NoEpilogue());
          } else {
            ASDF_STAGE(8, 0, 0, acc, h1, S0 + t * 2 + 0, epi);
            ASDF_STAGE(8, 1, 1, acc, h1, S0 + t * 2 + 1, NoEpilogue());
          }
        }

        // ---- layer 3 (512 -> 512) fused with layer 4 (dot with w4) and tanh
        float part = 0.0f;
        f32x16 acc3[2];
        auto dot_w4 = [&](const f32x16 a, int t) {
          const f32x4* w4 = reinterpret_cast<const f32x4*>(hc + CL::kW4 + t * 32 + hoff());
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const f32x4 w = w4[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              part = fmaf(relu_bit(a[c * 4 + r], 16 * (t & 1) + c * 4 + r, m3[t >> 1]), w[r], part);
            }
          }
          asm volatile("" : "+v"(m3[t >> 1]));      // (as in relu16m)
        };
#pragma unroll
        for (int t = 0; t < kTilesHidden; ++t) {
          f32x16& acc = acc3[t & 1];
          acc = load_bias16(hc + CL::kB3 + t * 32 + hoff());
          auto epi = [&]() {
            if (t > 0) {
              dot_w4(acc3[(t - 1) & 1], t - 1);
            } else {
              h2[kTilesHidden - 1] = relu16m(acc2[(kTilesHidden - 1) & 1], (kTilesHidden - 1) & 1, m2[(kTilesHidden - 1) >> 1]);
            }
          };
          constexpr int S0 = kStagesL1 + kStagesL2;
          ASDF_STAGE(16, 0, 0, acc, h2, S0 + t * 4 + 0, epi);
          ASDF_STAGE(16, 1, 1, acc, h2, S0 + t * 4 + 1, NoEpilogue());
          ASDF_STAGE(16, 2, 2, acc, h2, S0 + t * 4 + 2, NoEpilogue());
          ASDF_STAGE(16, 3, 3, acc, h2, S0 + t * 4 + 3, NoEpilogue());
        }
        dot_w4(acc3[(kTilesHidden - 1) & 1], kTilesHidden - 1);
        part += __shfl_xor(part, 32);
        const float sdf = tanhf(part + hc[CL::kB4]);
        if (valid && half == 0) {
          float* so = head == 0 ? p.sdf0 : p.sdf1;
          if (so) so[pi] = sdf;
        }
        if constexpr (LOSS) {
          // the loss term and its weight (both lane halves hold the point's value; half 0 counts it); a padding column is a point
          // outside the set
          float t = __int_as_float(0x7fc00000);
          if (valid) t = wgt[pi];
          const float c = q.clamp;
          const bool in_set = t == t;
          const float r = __fsub_rn(fminf(fmaxf(sdf, -c), c), fminf(fmaxf(t, -c), c));
          auto inv_n = [&]() -> float { return head ? q.inv_n[1] : q.inv_n[0]; };      // (selected at each use)
          const float sgn = r > 0.0f ? inv_n() : (r < 0.0f ? -inv_n() : 0.0f);
          const double l = half_sum_f64(in_set && half == 0 ? (double)fabsf(r) : 0.0);
          if (lane == 0) lsum[wave] += l;
          wp = (!in_set || sdf < -c || sdf > c) ? 0.0f : sgn;
        }
        // u = w (1 - s^2), the gradient kernel's form; 0 in a padding column (wp = 0 there)
        u = valid ? __fmul_rn(wp, __fsub_rn(1.0f, __fmul_rn(sdf, sdf))) : 0.0f;
      }

      // ================= reverse phase =================
      constexpr int R0 = kStagesHead;
      const float* w4h = hc + CL::kW4 + half * 16;        // w4 of (tile t, this lane half, register r): w4h[32 t + r]
      const int lane_row = tile_row(lane & 15, half);     // the row (within a tile) whose sums this lane carries into the sum block
      f32x4 keep = {0.f, 0.f, 0.f, 0.f};
      auto no_grp = [](int) { return f32x4{0.f, 0.f, 0.f, 0.f}; };
      auto no_epi = [](int) {};
#define ASDF_STAGE_V(Q, SLOT, ACC, GRP, BOP, SIDX, EPI) \
  stage_v<Q, SLOT>(ACC, GRP, BOP, ring, src_of((SIDX) + 3), lds_ring_base, lane, wave, a0, a1, EPI)

      // ---- d2 = (W3^T d3) * m2.  d3 is made inside the stages: K-step s = 16 tin + r reads bit (tin, r) of m3 and w4 of that row.
      // Tile t-1 is masked behind the first group of tile t and reduced (layer-2 rows), one register behind each group of stage 0.
      f32x16 d2[kTilesHidden];
      f32x16 accr[2];
      const float* w4t = w4h;
      auto w4_grp = [&](int q) {
        return [&, q](int g) { return *reinterpret_cast<const f32x4*>(w4t + (q * 4 + (g >> 2)) * 32 + (g & 3) * 4); };
      };
      auto d3_bop = [&](int s, const f32x4& wv) { return keep_if(__fmul_rn(u, wv[s & 3]), m3[s >> 5], s & 31); };
      float* rows2 = mysums + kHidden * kVjpRowFloats;
#pragma unroll
      for (int t = 0; t < kTilesHidden; ++t) {
        f32x16& acc = accr[t & 1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        // (the bit tests of m3 are the same in every tile: left visible, they are made once and their 256 lane masks kept in scalar registers)
#pragma unroll
        for (int i = 0; i < kTilesHidden / 2; ++i) asm volatile("" : "+v"(m3[i]));
        {
          // (and w4's LDS addresses are made per tile: hoisted out of the tile loop, they are spilled across it)
          w4t = hc + CL::kW4 + hoff();
        }
        auto epi = [&](int g) {
          if (t == 0) return;
          if (g == 0) d2[t - 1] = mask_tile(accr[(t - 1) & 1], m2[(t - 1) >> 1], (t - 1) & 1);
          reduce_reg(d2[t - 1][g], g, lane, x0, x1, x2, keep);
          if (g == 15) reduce_flush(keep, t - 1, lane_row, rows2);
        };
        ASDF_STAGE_V(0, 0, acc, w4_grp(0), d3_bop, R0 + t * 4 + 0, epi);
        ASDF_STAGE_V(1, 1, acc, w4_grp(1), d3_bop, R0 + t * 4 + 1, no_epi);
        ASDF_STAGE_V(2, 2, acc, w4_grp(2), d3_bop, R0 + t * 4 + 2, no_epi);
        ASDF_STAGE_V(3, 3, acc, w4_grp(3), d3_bop, R0 + t * 4 + 3, no_epi);
      }

      // ---- d1 = (W2a^T d2) * m1: 512 -> 256; the last d2 tile is finished inside the first d1 tile (its K-steps are >= 240)
      f32x16 d1[kTilesL1];
      f32x16 accs[2];
      auto d2_bop = [&](int s, const f32x4&) { return d2[s >> 4][s & 15]; };
#pragma unroll
      for (int t = 0; t < kTilesL1; ++t) {
        f32x16& acc = accs[t & 1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        auto epi = [&](int g) {
          if (t > 0) {
            if (g == 0) d1[t - 1] = mask_tile(accs[(t - 1) & 1], m1[(t - 1) >> 1], (t - 1) & 1);
          } else {
            if (g == 0) d2[kTilesHidden - 1] = mask_tile(accr[(kTilesHidden - 1) & 1], m2[(kTilesHidden - 1) >> 1], (kTilesHidden - 1) & 1);
            reduce_reg(d2[kTilesHidden - 1][g], g, lane, x0, x1, x2, keep);
            if (g == 15) reduce_flush(keep, kTilesHidden - 1, lane_row, rows2);
          }
        };
        constexpr int S0 = R0 + kStagesL3;
        ASDF_STAGE_V(0, 0, acc, no_grp, d2_bop, S0 + t * 4 + 0, epi);
        ASDF_STAGE_V(1, 1, acc, no_grp, d2_bop, S0 + t * 4 + 1, no_epi);
        ASDF_STAGE_V(2, 2, acc, no_grp, d2_bop, S0 + t * 4 + 2, no_epi);
        ASDF_STAGE_V(3, 3, acc, no_grp, d2_bop, S0 + t * 4 + 3, no_epi);
      }

      // ---- d0 = (W1^T d1) * m0: 256 -> 512, never stored: tile t-1 is masked and reduced (layer-0 rows) inside tile t
      f32x16 acct[2];
      f32x16 d0;
      auto d1_bop = [&](int s, const f32x4&) { return d1[s >> 4][s & 15]; };
#pragma unroll
      for (int t = 0; t < kTilesHidden; ++t) {
        f32x16& acc = acct[t & 1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        auto epi = [&](int g) {
          if (t > 0) {
            if (g == 0) d0 = mask_tile(acct[(t - 1) & 1], m0[(t - 1) >> 1], (t - 1) & 1);
            reduce_reg(d0[g], g, lane, x0, x1, x2, keep);
            if (g == 15) reduce_flush(keep, t - 1, lane_row, mysums);
          } else {
            if (g == 0) d1[kTilesL1 - 1] = mask_tile(accs[(kTilesL1 - 1) & 1], m1[(kTilesL1 - 1) >> 1], (kTilesL1 - 1) & 1);   // K-steps >= 112
          }
        };
        constexpr int S0 = R0 + kStagesL3 + kStagesL1;
        if (t & 1) {
          ASDF_STAGE_V(0, 2, acc, no_grp, d1_bop, S0 + t * 2 + 0, epi);
          ASDF_STAGE_V(1, 3, acc, no_grp, d1_bop, S0 + t * 2 + 1, no_epi);
        } else {
          ASDF_STAGE_V(0, 0, acc, no_grp, d1_bop, S0 + t * 2 + 0, epi);
          ASDF_STAGE_V(1, 1, acc, no_grp, d1_bop, S0 + t * 2 + 1, no_epi);
        }
      }
      d0 = mask_tile(acct[(kTilesHidden - 1) & 1], m0[(kTilesHidden - 1) >> 1], (kTilesHidden - 1) & 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) reduce_reg(d0[r], r, lane, x0, x1, x2, keep);
      reduce_flush(keep, kTilesHidden - 1, lane_row, mysums);
#undef ASDF_STAGE_V
#undef ASDF_STAGE
    }   // tiles

    // the four waves' sums, in wave order, into this workgroup's partial of the head
    __syncthreads();
    {
      float* out = v.partial + ((size_t)wg() * kHeads + head) * kVjpHeadFloats;
      // (the thread index is made again from the lane count: kept, it is one more register live across the tile loop)
      const int tid2 = wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      for (int i = tid2; i < kVjpHeadFloats; i += 256) {
        float s = sums[i];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s = __fadd_rn(s, sums[w * kVjpHeadFloats + i]);
        out[i] = s;
      }
      if constexpr (LOSS) {
        if (tid2 == 0) {
          double s = lsum[0];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) s += lsum[w];
          q.partial[(size_t)wg() * kHeads + head] = s;
        }
      }
    }
  }   // MLPs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The loss form's kernel body: workgroup blockIdx.x of the launch is workgroup b.wgs[blockIdx.x].g of sample
// b.wgs[blockIdx.x].sample.  The two words and the sample's descriptor are read with uniform addresses and held in scalar registers
// (nothing is written through them: descriptors are read-only to this kernel); p.xyz, v.w[] are the concatenated lists of the batch,
// v.partial / q.partial the rows of the whole launch, and the sample's share of each starts at its first point / first workgroup.
__device__ __forceinline__ void sdf_mlp_vjp_batch_body(const DecodeParams& p, const VjpParams& v, const VjpLossParams& q, const VjpBatchParams& b) {
  using CL = CstLayout<2>;
  const FitWg w = b.wgs[blockIdx.x];
  const int s = uniform_i(w.sample), g = uniform_i(w.g);
  const FitSampleDesc* sd = b.samples + s;
  const long long first = uniform_i(sd->first);
  const int m = uniform_i(sd->m), grid = uniform_i(sd->grid), wg0 = uniform_i(sd->wg0), mask = uniform_i(sd->heads_mask);
  DecodeParams ps = p;
  ps.P = m;
  ps.xyz = p.xyz + first * 3;
  ps.cst = b.cst + (size_t)s * kHeads * CL::kFloats;
  ps.first_mlp = (mask & 1) ? 0 : 1;
  ps.num_mlps = mask == 3 ? 2 : 1;
  VjpParams vs = v;
  vs.w[0] = v.w[0] + first;            // (a head outside the sample's mask is not evaluated: its list is never read)
  vs.w[1] = v.w[1] + first;
  vs.partial = v.partial + (size_t)wg0 * kVjpFoldFloats;
  VjpLossParams qs = q;
  qs.inv_n[0] = __int_as_float(uniform_i(__float_as_int(sd->inv_n[0])));
  qs.inv_n[1] = __int_as_float(uniform_i(__float_as_int(sd->inv_n[1])));
  qs.partial = q.partial + (size_t)wg0 * kHeads;
  sdf_mlp_vjp_body<true>(ps, vs, qs, (unsigned)g, (unsigned)grid);
}

// d_fold [2 heads][2 layers][512][4] = the workgroups' partials added in workgroup order (fp64 accumulator); a head that was not
// evaluated (bit `head` of heads_mask clear) is written with zeros.  One thread per entry: entry e of it.
__device__ __forceinline__ void vjp_reduce_entry(const float* __restrict__ partial, int grid, int heads_mask, float* __restrict__ d_fold, int e) {
  const int head = e / kVjpHeadFloats;
  double s = 0.0;
  if ((heads_mask >> head) & 1)
    for (int g = 0; g < grid; ++g) s += (double)partial[(size_t)g * kVjpFoldFloats + e];
  d_fold[e] = (float)s;
}

// The adjoint of fold_sample_kernel on d_fold (c = b + W_lat z + W_pt E[:, 3], A[:, d] = W_pt E[:, d]), workgroup `blk` of it:
//   d_latent[k]      = sum over (head, layer, row) of wlat[head][layer][row][k] dc[row]                      blocks [0, 64): 4 k each
//   d_embed[h][f][d] = sum over (layer, row) of wpt[h][layer][row][f] (d < 3 ? dA[row][d] : dc[row])          blocks 64 + h MAXPF + f
// fp64 accumulators; a thread's terms in index order, then a fixed tree over the 256 threads.  Either output may be null.
__device__ __forceinline__ void vjp_adjoint_body(const float* __restrict__ d_fold, const float* __restrict__ wlat, const float* __restrict__ wpt,
                                                 int max_pf, float* __restrict__ d_latent, float* __restrict__ d_embed, unsigned blk) {
  __shared__ double red[256][4];
  const int tid = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  const bool lat = blk < kLatent / 4;
  if (lat) {
    if (!d_latent) return;
    const int k4 = blk * 4;
    for (int j = tid; j < kHeads * 2 * kHidden; j += 256) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wlat + (size_t)j * kLatent + k4);
      const double dc = (double)d_fold[j * kVjpRowFloats + 3];
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] += (double)w[c] * dc;
    }
  } else {
    if (!d_embed) return;
    const int hf = blk - kLatent / 4, h = hf / max_pf, f = hf % max_pf;
    for (int j = h * 2 * kHidden + tid; j < (h + 1) * 2 * kHidden; j += 256) {
      const double w = (double)wpt[(size_t)j * max_pf + f];
      const f32x4 dv = *reinterpret_cast<const f32x4*>(d_fold + j * kVjpRowFloats);
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] += w * (double)dv[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) red[tid][c] = a[c];
  __syncthreads();
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[tid][c] += red[tid + n][c];
    __syncthreads();
  }
  if (tid < 4) {
    if (lat) d_latent[blk * 4 + tid] = (float)red[0][tid];
    else d_embed[(size_t)(blk - kLatent / 4) * 4 + tid] = (float)red[0][tid];
  }
}

// The data term of one step: per evaluated head the workgroups' fp64 sums in workgroup order, times 1 / n of the head, hand first
// (one thread).
__device__ __forceinline__ void vjp_loss_total(const double* __restrict__ loss_partial, int grid, int heads_mask, double inv_n0, double inv_n1,
                                               double* __restrict__ history) {
  double total = 0.0;
  for (int head = 0; head < kHeads; ++head) {
    if (!((heads_mask >> head) & 1)) continue;
    double s = 0.0;
    for (int g = 0; g < grid; ++g) s += loss_partial[(size_t)g * kHeads + head];
    total += s * (head == 0 ? inv_n0 : inv_n1);
  }
  *history = total;
}

// The Adam state of one code (k1_launch.h: [z | m | v | d_latent | z0][kLatent]), a lane per entry: its start ...
__device__ __forceinline__ void adam_init_body(float* __restrict__ state, const float* __restrict__ z, const float* __restrict__ z0) {
  const int i = threadIdx.x;
  if (i >= kLatent) return;
  const float zi = z[i];
  state[i] = zi;
  state[kLatent + i] = 0.0f;
  state[2 * kLatent + i] = 0.0f;
  state[3 * kLatent + i] = 0.0f;
  state[4 * kLatent + i] = z0 ? z0[i] : zi;
}

// ... and one step.  (sqrtf and the division below are the compiler's correctly rounded forms - the default of this toolchain for fp32,
// and what fit.adam_step_host's numpy operations are; __fsqrt_rn maps to the approximate instruction here.  The units are built without
// contraction, so no product is fused into a sum.)
__device__ __forceinline__ void adam_step_body(float* __restrict__ state, const float* __restrict__ step, const AdamRule& r, float* __restrict__ z_out) {
  const int i = threadIdx.x;
  if (i >= kLatent) return;
  const float a = step[0], s = step[1];
  float z = state[i], m = state[kLatent + i], v = state[2 * kLatent + i];
  const float g = __fadd_rn(state[3 * kLatent + i], __fmul_rn(r.k_prior, __fsub_rn(z, state[4 * kLatent + i])));
  m = __fadd_rn(__fmul_rn(r.b1, m), __fmul_rn(__fsub_rn(1.0f, r.b1), g));
  v = __fadd_rn(__fmul_rn(r.b2, v), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, r.b2), g), g));
  const float den = __fadd_rn(__fmul_rn(sqrtf(v), s), r.eps);
  z = __fsub_rn(z, __fmul_rn(a, m / den));
  state[i] = z;
  state[kLatent + i] = m;
  state[2 * kLatent + i] = v;
  z_out[i] = z;
}

}  // namespace asdf
