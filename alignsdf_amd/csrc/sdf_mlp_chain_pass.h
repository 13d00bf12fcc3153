// One pass of the fp32 chain, sdf_mlp_body<0, 2, false>'s tile body, for the columns of a wave: layers 0 to 3, the fused last-layer
// dot product, the LDS ring and the stage schedule.  A BODY FRAGMENT: no #pragma once, no namespace - it is included inside a function,
// where the pass stands (sdf_mlp_grad_body, sdf_mlp_project_body, sdf_mlp_trace_body), once per function.
//
// Reads from the including scope:
//   hc, ring, lds_ring_base, sbase0, lane, wave, half    the head's constants block, the weight ring and its source, who I am
//   x0, x1, x2                                           the point this column feeds
//   a0, a1                                               the first A operands of the next stage (read and written: they travel from
//                                                        pass to pass, as from tile to tile in sdf_mlp_body)
//   KP, CL                                               2 and CstLayout<2>
//   and whatever the includer's hooks name (the gradient form's `tangent`).
// Defines: part, the column's last-layer dot product without the bias b4, summed over both lane halves.  (bp, sbase, src_of, h0 .. h2,
// acc1 .. acc3 and dot_w4 are its own, and visible after it like any local of the enclosing block.)
// Hooks, defined by the includer before the #include and undefined after it:
//   ASDF_CHAIN_BIAS(P)      f32x16: the accumulators' start from the bias block at P
//   ASDF_CHAIN_RELU16(V)    f32x16: a tile's activation
//   ASDF_CHAIN_RELU(V)      float: one row's activation, in the last-layer dot product
// ASDF_STAGE is defined and undefined here.  The tile index is `tl`: `t` is the ray parameter of the tracing body.
//
// Three texts of the chain remain: sdf_mlp_body (sdf_mlp_kernel.h, with its ablation / NeRF / two-output / classifier / pixel-aligned
// openings), this fragment, and the forward phase of sdf_mlp_vjp_body (it keeps a ReLU mask per register).  A change to the ring, the
// waits or the stage schedule is made in those three places.
//
// Why a fragment and not a function: the preprocessor pastes the same tokens into the same scope, and the three units compile to the
// assembly they had when each carried its own copy (tools/isa_fingerprint.py).  As a __device__ __forceinline__ template function, with
// the bias / ReLU policy as a struct or as static members, the generated code changes under the shipped per-unit flags: the gradient
// kernel goes from 256 + 229 registers and no scratch to 256 + 256 and 2240 B of scratch per lane, the tracing kernel from 256 + 247
// and none to 256 + 256 and 1392 B.  The MFMA count and the optimised IR's instruction mix are the same in both forms; what differs
// is where the loop-invariant LDS address computations end up, which is what these kernels depend on (the opaque sbase below, hoff() in
// sdf_mlp_vjp_kernel.h).  Lifetime markers are not the cause: -Xclang -disable-lifetime-markers changes nothing.

      // B operands of the point-feature K-steps: lane half h supplies feature 2 s + h of K-step s
      float bp[KP];
      bp[0] = half ? x1 : x0;
      bp[1] = half ? 0.0f : x2;
      const float* sbase = sbase0;
      asm volatile("" : "+s"(sbase));
      auto src_of = [&](int s) -> const float* {   // s = stage index within the head + 3
        return sbase + (size_t)(s < kStagesHead ? s : s - kStagesHead) * kStageFloats;
      };

      // ---- layer 0
      f32x16 h0[kTilesHidden];
#pragma unroll
      for (int tl = 0; tl < kTilesHidden; ++tl) {
        f32x16 acc = ASDF_CHAIN_BIAS(hc + CL::kC0 + (tl * 2 + half) * 16);
#pragma unroll
        for (int s = 0; s < KP; ++s) acc = ASDF_MFMA(hc[CL::kA0 + (tl * KP + s) * 64 + lane], bp[s], acc);
        h0[tl] = ASDF_CHAIN_RELU16(acc);
      }

#define ASDF_STAGE(KT, Q, SLOT, ACC, HIN, SIDX, EPI) \
  stage<KT, Q, SLOT, 0>(ACC, HIN, ring, src_of((SIDX) + 3), lds_ring_base, lane, wave, a0, a1, EPI)

      // ---- layer 1: 512 -> 256; epilogue of tile tl-1 rides in tile tl
      f32x16 h1[kTilesL1];
      f32x16 acc1[2];
#pragma unroll
      for (int tl = 0; tl < kTilesL1; ++tl) {
        f32x16& acc = acc1[tl & 1];
        acc = ASDF_CHAIN_BIAS(hc + CL::kB1 + (tl * 2 + half) * 16);
        auto epi = [&]() {
          if (tl == 0) return;
          h1[tl - 1] = ASDF_CHAIN_RELU16(acc1[(tl - 1) & 1]);
        };
        ASDF_STAGE(16, 0, 0, acc, h0, tl * 4 + 0, epi);
        ASDF_STAGE(16, 1, 1, acc, h0, tl * 4 + 1, NoEpilogue());
        ASDF_STAGE(16, 2, 2, acc, h0, tl * 4 + 2, NoEpilogue());
        ASDF_STAGE(16, 3, 3, acc, h0, tl * 4 + 3, NoEpilogue());
      }

      // ---- layer 2: [h1 (256) | xyz (4)] -> 512
      f32x16 h2[kTilesHidden];
      f32x16 acc2[2];
#pragma unroll
      for (int tl = 0; tl < kTilesHidden; ++tl) {
        f32x16& acc = acc2[tl & 1];
        acc = ASDF_CHAIN_BIAS(hc + CL::kC2 + (tl * 2 + half) * 16);
#pragma unroll
        for (int s = 0; s < KP; ++s) acc = ASDF_MFMA(hc[CL::kA2 + (tl * KP + s) * 64 + lane], bp[s], acc);
        auto epi = [&]() {
          if (tl > 0) h2[tl - 1] = ASDF_CHAIN_RELU16(acc2[(tl - 1) & 1]);
          else h1[kTilesL1 - 1] = ASDF_CHAIN_RELU16(acc1[(kTilesL1 - 1) & 1]);   // consumed by K-steps >= 112
        };
        constexpr int S0 = kStagesL1;
        if (tl & 1) {
          ASDF_STAGE(8, 0, 2, acc, h1, S0 + tl * 2 + 0, epi);
          ASDF_STAGE(8, 1, 3, acc, h1, S0 + tl * 2 + 1, NoEpilogue());
        } else {
          ASDF_STAGE(8, 0, 0, acc, h1, S0 + tl * 2 + 0, epi);
          ASDF_STAGE(8, 1, 1, acc, h1, S0 + tl * 2 + 1, NoEpilogue());
        }
      }

      // ---- layer 3 (512 -> 512) fused with layer 4 (dot with w4)
      float part = 0.0f;
      f32x16 acc3[2];
      auto dot_w4 = [&](const f32x16 a, int tl) {
        const f32x4* w4 = reinterpret_cast<const f32x4*>(hc + CL::kW4 + (tl * 2 + half) * 16);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 w = w4[c];
#pragma unroll
          for (int r = 0; r < 4; ++r) part = fmaf(ASDF_CHAIN_RELU(a[c * 4 + r]), w[r], part);
        }
      };
#pragma unroll
      for (int tl = 0; tl < kTilesHidden; ++tl) {
        f32x16& acc = acc3[tl & 1];
        acc = ASDF_CHAIN_BIAS(hc + CL::kB3 + (tl * 2 + half) * 16);
        auto epi = [&]() {
          if (tl > 0) dot_w4(acc3[(tl - 1) & 1], tl - 1);
          else h2[kTilesHidden - 1] = ASDF_CHAIN_RELU16(acc2[(kTilesHidden - 1) & 1]);   // consumed by K-steps >= 240
        };
        constexpr int S0 = kStagesL1 + kStagesL2;
        ASDF_STAGE(16, 0, 0, acc, h2, S0 + tl * 4 + 0, epi);
        ASDF_STAGE(16, 1, 1, acc, h2, S0 + tl * 4 + 1, NoEpilogue());
        ASDF_STAGE(16, 2, 2, acc, h2, S0 + tl * 4 + 2, NoEpilogue());
        ASDF_STAGE(16, 3, 3, acc, h2, S0 + tl * 4 + 3, NoEpilogue());
      }
      dot_w4(acc3[(kTilesHidden - 1) & 1], kTilesHidden - 1);
#undef ASDF_STAGE
      part += __shfl_xor(part, 32);
