// K1T: sphere tracing on the fp32 chain (sdf_mlp_kernel.h) - every MFMA column marches one ray, and a column whose ray is done takes
// the next ray from a queue at the next step boundary.
//
// The columns of an MFMA do not interact, so "the same 128 columns again" is, to the weight ring, the next tile (src_of wraps as in
// sdf_mlp_body) and the point a column feeds may change freely between two passes of the chain.  A column holds one ray's state in
// registers (both lane halves of a column carry the same copy: they see the same sdf bits, so they stay equal without talking).
// One iteration = refill the free columns, vote, form p = o + t d, one pass of the chain (sdf_mlp_chain_pass.h, the text the gradient
// and projection bodies include too: sdf_mlp_body<0, 2, false>'s tile body; a change to the ring, the waits or the stage schedule is
// made there, in sdf_mlp_body and in the forward phase of sdf_mlp_vjp_body), update the state by the rule below.  The value of a column goes through the operations of sdf_mlp_body<0, 2, false> on the same
// operands: at every point the kernel samples, its sdf is asdf_decode_points' under ASDF_MATH_F32, bit for bit.
//
// The rule (all fp32, every operation rounded on its own; per ray and head; TraceRule below):
//   start    o, d, t0, t1 not all finite, or t0 > t1: MISS with 0 evaluations.  Else t = t0, MARCH.
//   MARCH    sample f at t.
//            f <= 0: the ray's first sample -> INSIDE, t_out = t0.  Else the bracket is (t_prev, f_prev) .. (t, f) -> REFINE with
//                    r = refine_steps (r == 0: finish at once).
//            f > 0:  (t_prev, f_prev) = (t, f); t == t1 -> MISS (the end of the segment is always sampled, exactly); else count the
//                    march: count == max_steps -> EXHAUSTED, t_out = t; else t = min(t + clamp(step_scale f, min_step, max_step), t1).
//   REFINE   the midpoint tm = 0.5 (t_lo + t_hi); tm equal to an end -> finish (it is not sampled).  Sample f at tm: f <= 0 replaces
//            the hi end, else the lo end; r -= 1; r == 0 -> finish.
//   finish   t_out = clamp(t_lo + (t_hi - t_lo) (f_lo / (f_lo - f_hi)), t_lo, t_hi), correctly rounded division; HIT.
//   (min / clamp are written with comparisons, "x < hi ? x : hi": a NaN sample steps by min_step, a NaN position ends the march at t1.)
// Every ray takes at most max_steps + refine_steps + 1 evaluations and the queue is finite: the loop is bounded by construction, and
// no workgroup waits for another.
//
// A header of its own, not a template parameter of sdf_mlp_body: every other unit compiles from unchanged text.
#pragma once
#include "k1_launch.h"
#include "sdf_mlp_kernel.h"

namespace asdf {

enum TraceStatus : int { kTraceMiss = 0, kTraceHit = 1, kTraceInside = 2, kTraceExhausted = 3 };
enum TracePhase : int { kPhaseIdle = 0, kPhaseMarch = 1, kPhaseRefine = 2 };

// the workgroup vote's words live behind the constants block (dynamic LDS: no static LDS shifts the ring's base)
constexpr int kTraceLdsBytes = kLdsBytes + 2 * kWaves * (int)sizeof(int);

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// p.stream / p.cst / p.first_mlp / p.num_mlps as for sdf_mlp_body (KP == 2, SeparateDecoder); everything else in TraceParams
__device__ __forceinline__ void sdf_mlp_trace_body(const DecodeParams& p, const TraceParams& q) {
  constexpr int KP = 2;
  using CL = CstLayout<KP>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;
  float* cst = smem + kLdsRingFloats;
  int* vote = reinterpret_cast<int*>(cst + CL::kFloats);      // [2][kWaves]: "a column of wave w is live", by iteration parity

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;

  const long long M = q.M;
  const unsigned lds_ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;

#pragma unroll 1
  for (int slot = 0; slot < p.num_mlps; ++slot) {
    const int head = p.first_mlp + slot;
    const float* hc = cst;
    const TraceOutputs out = q.out[head];
    unsigned long long* queue = q.queue + head;
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

    // ---- this column's ray (t_lo / f_lo are t_prev / f_prev while it marches)
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
    float t = 0.f, t1 = 0.f, tlo = 0.f, flo = 0.f, thi = 0.f, fhi = 0.f;
    int phase = kPhaseIdle, count = 0, evals = 0;      // count: marches taken (MARCH) / refinements left (REFINE)
    long long ray = 0;
    bool want = true;                                   // the column is free and the queue may still hold a ray for it

    // a finished ray: its outputs (one lane per column writes), and the column is free again
    auto retire = [&](int status, float tout) {
      if (half == 0) {
        if (out.t) out.t[ray] = tout;
        if (out.status) out.status[ray] = status;
        if (out.evals) out.evals[ray] = evals;
        if (out.bracket) {
          const bool hit = status == kTraceHit;
          reinterpret_cast<f32x4*>(out.bracket)[ray] = f32x4{hit ? tlo : 0.0f, hit ? thi : 0.0f, hit ? flo : 0.0f, hit ? fhi : 0.0f};
        }
      }
      phase = kPhaseIdle;
      want = true;
    };
    // the bracket is final
    auto finish = [&]() {
      const float w = __fdiv_rn(flo, __fsub_rn(flo, fhi));
      float tout = __fadd_rn(tlo, __fmul_rn(__fsub_rn(thi, tlo), w));
      tout = tout > tlo ? tout : tlo;
      tout = tout < thi ? tout : thi;
      retire(kTraceHit, tout);
    };
    // the next REFINE sample, or the end of the refinement
    auto refine_next = [&]() {
      const float tm = __fmul_rn(0.5f, __fadd_rn(tlo, thi));
      if (count == 0 || tm == tlo || tm == thi) finish();
      else t = tm;
    };

#pragma unroll 1
    for (int iter = 0;; ++iter) {
      // ---- refill: free columns take the next rays of the queue - one aggregated atomic per wave and round, indices by lane prefix.
      // A ray that is over before its first sample (a MISS at the start) frees its column again, hence the loop: every round
      // consumes queue indices, and a column that draws one >= M never asks again.
      while (true) {
        const unsigned asking = (unsigned)__ballot(want);          // (both halves of a column agree: the low word says it all)
        if (asking == 0) break;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(queue, (unsigned long long)__popc(asking));
        base = __shfl(base, 0);
        if (want) {
          ray = (long long)(base + (unsigned long long)__popc(asking & ((1u << col) - 1u)));
          want = false;
          if (ray < M) {
            const f32x4* r4 = reinterpret_cast<const f32x4*>(q.rays) + ray * 2;
            const f32x4 ra = r4[0], rb = r4[1];
            o0 = ra[0]; o1 = ra[1]; o2 = ra[2]; d0 = ra[3]; d1 = rb[0]; d2 = rb[1];
            t = rb[2]; t1 = rb[3];
            evals = 0; count = 0;
            tlo = flo = thi = fhi = 0.0f;
            const bool ok = finite_f(o0) && finite_f(o1) && finite_f(o2) && finite_f(d0) && finite_f(d1) && finite_f(d2) &&
                            finite_f(t) && finite_f(t1) && !(t > t1);
            if (ok) phase = kPhaseMarch;
            else retire(kTraceMiss, __int_as_float(0x7f800000));
          }
        }
      }
      // ---- the workgroup leaves the head when every one of its columns is idle (uniform: the stage barriers below need all four
      // waves on the same trip count).  Two sets of words by parity: a wave that is an iteration ahead writes the other set.
      const bool live = phase != kPhaseIdle;
      int* votes = vote + (iter & 1) * kWaves;
      const int wave_live = __ballot(live) != 0 ? 1 : 0;          // (asked of the whole wave, not under the lane test below)
      if (lane == 0) votes[wave] = wave_live;
      __syncthreads();
      if ((votes[0] | votes[1] | votes[2] | votes[3]) == 0) break;

      // ---- the sample point (an idle column feeds zeros)
      float x0 = 0.f, x1 = 0.f, x2 = 0.f;
      if (live) {
        x0 = __fadd_rn(o0, __fmul_rn(t, d0));
        x1 = __fadd_rn(o1, __fmul_rn(t, d1));
        x2 = __fadd_rn(o2, __fmul_rn(t, d2));
      }
      // one pass of the chain: sdf_mlp_body<0, 2, false>'s bias and ReLU
#define ASDF_CHAIN_BIAS(P) load_bias16(P)
#define ASDF_CHAIN_RELU16(V) relu16i(V)
#define ASDF_CHAIN_RELU(V) __int_as_float(max(__float_as_int(V), 0))
#include "sdf_mlp_chain_pass.h"
#undef ASDF_CHAIN_BIAS
#undef ASDF_CHAIN_RELU16
#undef ASDF_CHAIN_RELU
      const float f = tanhf(part + hc[CL::kB4]);

      // ---- the rule
      if (live) {
        ++evals;
        if (phase == kPhaseMarch) {
          if (f <= 0.0f) {
            if (evals == 1) {
              retire(kTraceInside, t);
            } else {
              thi = t; fhi = f;
              count = q.rule.refine_steps;
              phase = kPhaseRefine;
              refine_next();
            }
          } else {
            tlo = t; flo = f;
            if (t == t1) {
              retire(kTraceMiss, __int_as_float(0x7f800000));
            } else if (++count == q.rule.max_steps) {
              retire(kTraceExhausted, t);
            } else {
              float s = __fmul_rn(q.rule.step_scale, f);
              s = s > q.rule.min_step ? s : q.rule.min_step;
              s = s < q.rule.max_step ? s : q.rule.max_step;
              const float tn = __fadd_rn(t, s);
              t = tn < t1 ? tn : t1;
            }
          }
        } else {
          if (f <= 0.0f) { thi = t; fhi = f; }
          else { tlo = t; flo = f; }
          --count;
          refine_next();
        }
      }
    }   // iterations
  }   // MLPs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace asdf
