// K1h: the fused SDF decoder with split-half arithmetic - the structure of sdf_mlp_kernel.h (register-resident
// activations, head-outer / tile-inner loop, 16 KiB weight stages through a 4-slot LDS-DMA ring, deferred epilogues),
// but the three hidden GEMMs run on v_mfma_f32_32x32x16_f16 instead of v_mfma_f32_32x32x2_f32:
//
//   every operand x is carried as two fp16 planes of x * S (S a power of two):  hi = fp16(x S),  lo = fp16(x S - hi),
//   i.e. 22 significand bits, and a product sum is three MFMAs into ONE fp32 accumulator:
//       acc += W_hi . x_lo + W_lo . x_hi + W_hi . x_hi          (the lo.lo term is < 2^-22 of the product)
//   fp16 x fp16 products are exact in fp32 and the accumulation is fp32, so the result is fp32-class (measured on the
//   synthetic decoders: max |error| vs fp64 2.8e-7, the same as the fp32 MFMA chain) at 3/16 of the MFMA time of the
//   fp32 instruction.  Scales: weights S_w per layer (max |w| S_w in [512, 1024)), activations S_x per MLP and layer,
//   calibrated by the host from the peak plane values a sweep leaves in the decoder's status record (default 8); biases and
//   the fp32 point-feature products enter the accumulator pre-multiplied by S_w S_x (pack.h, K0), and the accumulator is
//   rescaled by an exact power of two when it is split into the next layer's planes (the multipliers travel in the
//   constants block).  fp16 subnormal inputs are honoured by the MFMA (tools/mfma_f16_probe.hip), so small low planes
//   degrade gracefully.
//
// One body, four forms (template parameters of sdf_mlp_f16_body):
//   PL = 2            the split-half kernel above - the default arithmetic of every grid sweep;
//   PL = 2, SUB       the same over a list of lattice voxels (the values of the narrow-band fine sweep);
//   PL = 1, G = 1 | 2 one fp16 plane per operand, one MFMA per product sum, one or two 32-point groups per wave: the sweeps whose
//                     values are consumed through signs only (asdf_decode_grid_box / _band);
//   KP = 5 | 8        NeRF-encoded point features (k1h_nerf_kernels.hip).
//
// Operand maps (tools/mfma_f16_probe.hip): A lane l holds A[i = l & 31][k = 8 (l >> 5) + e], B lane l holds
// B[k = 8 (l >> 5) + e][j = l & 31], e = 0..7 packed in 4 VGPRs; D as the fp32 form.  Registers 8 s .. 8 s + 7 of an
// output tile are therefore, after the split, the B operand of K-block 2 tile + s of the next layer (the host packs
// the weight columns in that order).
#pragma once
#include <type_traits>

#include "sdf_mlp_kernel.h"

namespace asdf {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define ASDF_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

// 2 relu(a0, a1) -> one packed fp16 register (word `w` of an h8), as explicit 2-vectors: one v_cvt_pk_f16_f32 per pair (left to
// the SLP vectoriser the pairs came out shifted by one element, with a v_alignbit / v_pack per register on top)
// (The one-plane kernels' own image - decoder.hip: rebuild_one_plane - is scaled so that an accumulator carries its activation's
// plane scale: no multiply, and no running maximum either.)
// The ReLU of the folded image must PRESERVE a poisoned value.  The matrix pipe's inf - inf is a NEGATIVE NaN (0xffc00000,
// tools/trapsts_probe.hip), and an integer maximum against 0 - the cheapest ReLU - turns it (and a -inf) into a perfectly finite 0:
// measured, a layer-2 overflow of 512 x the fp16 range reached the output as a finite value.  So: convert first, then
//     2 relu(c) = c + |c|        (v_and_b32 0x7fff7fff + v_pk_add_f16)
// exact for finite halves (0 for negative ones, 2 c otherwise), and NaN + NaN = NaN, -inf + inf = NaN, inf + inf = inf: whatever left
// the fp16 range stays non-finite through every layer, reaches the output as a NaN or exactly +-1, and is reported there.  The factor
// 2 lives in the image's scales (decoder.hip: rebuild_one_plane carries S_x / 2 in the accumulators).  Three VALU instructions per
// register pair (round 3: five, with a running maximum that the 512-register budget has no room for: +39 % time when it spills).
__device__ __forceinline__ void relu_pack(float a0, float a1, h8& dst, int w) {
  f32x2 raw;
  raw[0] = a0; raw[1] = a1;
  const h2 c = __builtin_convertvector(raw, h2);
  const h2 m = __builtin_bit_cast(h2, __builtin_bit_cast(unsigned, c) & 0x7fff7fffu);
  const h2 r2 = c + m;
  u32x4 d0 = __builtin_bit_cast(u32x4, dst);
  d0[w] = __builtin_bit_cast(unsigned, r2);
  dst = __builtin_bit_cast(h8, d0);
}

// wave64 maximum of a signed int on the DPP network (row_shr 1 / 2 / 4 / 8 inside the rows of 16 lanes, row_bcast:15 / :31 across them);
// the result as a wave-uniform value (lane 63 holds it)
__device__ __forceinline__ int wave_max_i32(int v) {
#define ASDF_DPP_MAX(ctrl, rows) v = max(v, __builtin_amdgcn_update_dpp((int)0x80000000, v, (ctrl), (rows), 0xf, false))
  ASDF_DPP_MAX(0x111, 0xf); ASDF_DPP_MAX(0x112, 0xf); ASDF_DPP_MAX(0x114, 0xf); ASDF_DPP_MAX(0x118, 0xf);
  ASDF_DPP_MAX(0x142, 0xa); ASDF_DPP_MAX(0x143, 0xc);
#undef ASDF_DPP_MAX
  return __builtin_amdgcn_readlane(v, 63);
}

constexpr float kActScaleDev = 8.0f;   // S_x (pack.h: kActScale)

#ifndef ASDF16_STAGE_KB
#define ASDF16_STAGE_KB 16       // K-blocks per stage: 16 = 32 KiB stages (one barrier per 48 MFMAs), 8 = 16 KiB stages
#endif

// The split-half stream of a head is a flat sequence of (tile, K-block) records of 2 KiB ([plane hi / lo][lane][8 halves]),
// 1024 of them; a stage is ASDF16_STAGE_KB consecutive records of one tile, so the stage size is the kernel's choice.
//
// PL = number of fp16 planes per operand.  2 is the split-half arithmetic above.  1 keeps only the high plane - plain fp16
// operands, ONE MFMA per product sum, fp16-class results (errors of a few 1e-4 on the synthetic decoders): the kernel of
// the box-only coarse sweep (asdf_decode_grid_box), whose output is consumed only through the bounding box of its
// negative voxels and is re-evaluated exactly wherever that box could depend on the error.  Its weight stream is the
// high planes alone (1 KiB records), so a 16-K-block stage is 16 KiB.
constexpr int kS16Kb = ASDF16_STAGE_KB;
constexpr int kS16Head = 1024 / kS16Kb;              // stages per head
// G = point groups per wave (one-plane kernel only): with G = 2 a wave carries 64 points as two groups of 32 whose
// activations occupy the registers of the two planes of the split-half kernel; every A fragment read from LDS then feeds two
// MFMAs (one per group).  The one-plane kernel with one group is LDS-bandwidth-bound: four waves reading 1 KiB of A
// fragments per 32-cycle MFMA are exactly the 128 B / clk of the LDS, before the LDS-DMA writes.
template <int PL, int G = 1>
struct S16 {
  static constexpr int kFloats = kS16Kb * 256 * PL;        // floats per stage
  static constexpr int kPieces = kS16Kb * PL / 4;          // 1 KiB LDS-DMA pieces per wave per stage
  static constexpr int kWaveFloats = kFloats / kWaves;     // a wave's share of a stage
  static constexpr int kRingFloats = kRing * kFloats;
  static constexpr int kMfmas = PL == 2 ? 3 : G;           // MFMAs per K-block
  // A fragments are read from LDS this many K-blocks ahead of their MFMAs: the read latency (~100 cycles) has to fit in the
  // MFMA time of that distance - one K-block of three MFMAs (96 cycles), three K-blocks of one, or two K-blocks of two (64 cycles each)
  static constexpr int kPrefetch = PL == 2 ? 1 : (G == 2 ? 2 : 3);
  static_assert(PL == 2 ? G == 1 : (G == 1 || G == 2), "point groups");
  static_assert(kPieces == 4 || kPieces == 8, "stage size");
};
constexpr int kS16Floats = S16<2>::kFloats;
constexpr int kS16Pieces = S16<2>::kPieces;
constexpr int kS16WaveFloats = S16<2>::kWaveFloats;
constexpr int kRing16Floats = S16<2>::kRingFloats;
// LDS: ring + constants + two 8-int negative-voxel records per wave (the register file has no room for per-lane ones)
constexpr int kWrecInts = 20;    // per wave: two 8-int negative-voxel records + the largest plane value of layers 0..2 (+ pad)
// one-plane kernel (its K-blocks are 32 / 64 matrix-pipe cycles, not 96, so what hides behind a K-block of the split-half kernel does
// not hide there): point features and bias rows of layers 0 / 2 on ONE fp16 MFMA per tile (sdf_layout.h: kA16Floats)
constexpr bool pt16(int kp, int planes) { return planes == 1 && kp == 2; }
constexpr int lds_bytes_f16(int kp, int planes = 2) {
  return (kRing * kS16Kb * 256 * planes + cst_offsets(kp).floats + (pt16(kp, planes) ? kA16Floats : 0)) * 4 + kWaves * kWrecInts * 4;
}
constexpr int kLdsBytesF16 = lds_bytes_f16(2);
constexpr int kLdsBytesF16P1 = lds_bytes_f16(2, 1);
static_assert(kS16Kb == 8 || kS16Kb == 16, "stage size");

// relu(acc) * mul -> the two fp16 planes of K-blocks (2 t, 2 t + 1) of the next layer, element e (0..7) of each;
// amax tracks the largest value handed to the fp16 conversion (>= 65520 rounds to infinity: the caller reports it)
// (g: -1 = everything, 0 / 1 = only the first / second point group's part - the two-group kernel issues them behind different MFMAs)
template <int PL = 2, int G = 1, bool MIX = false>
__device__ __forceinline__ void split_part(const f32x16& acc, const f32x16& accb, float mul, h8& hi0, h8& lo0, h8& hi1, h8& lo1, float& amax,
                                           int e, int g = -1, int step = -1, float* rr = nullptr) {
  if (PL == 1 && G == 2 && g != 0)         // the second point group: its planes live where the low planes of the split-half kernel do
    relu_pack(accb[2 * e], accb[2 * e + 1], e < 4 ? lo0 : lo1, e & 3);
  if (PL == 1 && G == 2 && g == 1) return;
  if (PL == 1) {
    // one plane: part e converts the NEIGHBOURING accumulator registers 2 e, 2 e + 1 (both land in one packed fp16 register,
    // one v_cvt_pk), about 5 VALU instructions - a part has to fit the shadow of the ONE MFMA of its K-block here
    relu_pack(acc[2 * e], acc[2 * e + 1], e < 4 ? hi0 : hi1, e & 3);
    return;
  }
  if (MIX) {
  // Round 5: the split on the mixed-precision FMA.  v_fma_mix{lo,hi}_f16 computes an fp32 FMA whose sources are fp32 registers or
  // fp16 halves, rounds ONCE to fp16 and writes one half of the destination (the other half is preserved), so per element
  //     hi = f16(r mul)                 lo = f16(r mul - hi)        (r mul is exact: mul is a power of two; r mul - hi is exact in fp32)
  // are two instructions with no conversion back, no subtraction and no packing - the bits of the form below, which took
  // v_mul + v_fma_mixlo + v_cvt_f32_f16 + v_sub + 2 x 1/2 v_cvt_pk per element (17 VALU instructions per epilogue part, where the
  // part's K-block has room for ~12 next to its MFMAs, LDS reads and LDS-DMA piece).  The running maximum is taken on r and scaled
  // by mul once per tile (max and a positive power of two commute).
  // `step` (-1 = the whole part) issues the part in three pieces, one behind each MFMA of the part's K-block - [0] the two ReLUs (the
  // accumulator reads), [1] the high planes and the running maximum, [2] the low planes; rr[2] carries the ReLUs across.  A K-block is
  // three DEPENDENT MFMAs on one accumulator: an MFMA that finds more than ~5 issue slots between itself and its predecessor misses
  // the back-to-back window and pays ~43 clocks on top of the slots (MI355X_MICROARCH.md, "one EXTRA issue slot between two MFMAs on
  // the SAME accumulator"), which is why the instruction count of a part hardly matters while the part sits in ONE gap.
  {
    float r0 = rr ? rr[0] : 0.0f, r1 = rr ? rr[1] : 0.0f;
    if (step <= 0) {
      r0 = __int_as_float(max(__float_as_int(acc[e]), 0));
      r1 = __int_as_float(max(__float_as_int(acc[8 + e]), 0));
      if (rr) { rr[0] = r0; rr[1] = r1; }
      if (step == 0) return;
    }
    u32x4 H0 = __builtin_bit_cast(u32x4, hi0), L0 = __builtin_bit_cast(u32x4, lo0);
    u32x4 H1 = __builtin_bit_cast(u32x4, hi1), L1 = __builtin_bit_cast(u32x4, lo1);
    unsigned a = H0[e >> 1], b = L0[e >> 1], c = H1[e >> 1], d = L1[e >> 1];
    // the two high planes, the running maximum behind them, then the low planes (a half-register write needs two wait states in
    // front of its first read: the maximum and the sibling's instruction are those two)
    if (step != 2) {
      if (e & 1)
        asm("v_fma_mixhi_f16 %0, %3, %5, 0\n\t"
            "v_fma_mixhi_f16 %1, %4, %5, 0\n\t"
            "v_max3_f32 %2, %2, %3, %4\n\t"
            : "+v"(a), "+v"(c), "+v"(amax) : "v"(r0), "v"(r1), "v"(mul));
      else        // (the even element defines the register: nothing of the previous tile's value is read)
        asm("v_fma_mixlo_f16 %0, %3, %5, 0\n\t"
            "v_fma_mixlo_f16 %1, %4, %5, 0\n\t"
            "v_max3_f32 %2, %2, %3, %4\n\t"
            : "=&v"(a), "=&v"(c), "+v"(amax) : "v"(r0), "v"(r1), "v"(mul));
      H0[e >> 1] = a; H1[e >> 1] = c;
      hi0 = __builtin_bit_cast(h8, H0); hi1 = __builtin_bit_cast(h8, H1);
    }
    if (step != 1) {
      if (e & 1)
        asm("v_fma_mixhi_f16 %0, %2, %4, -%5 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %1, %3, %4, -%6 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "+v"(b), "+v"(d) : "v"(r0), "v"(r1), "v"(mul), "v"(a), "v"(c));
      else
        asm("v_fma_mixlo_f16 %0, %2, %4, -%5 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixlo_f16 %1, %3, %4, -%6 op_sel_hi:[0,0,1]"
            : "=&v"(b), "=&v"(d) : "v"(r0), "v"(r1), "v"(mul), "v"(a), "v"(c));
      L0[e >> 1] = b; L1[e >> 1] = d;
      lo0 = __builtin_bit_cast(h8, L0); lo1 = __builtin_bit_cast(h8, L1);
    }
    return;
  }
  }
  const float t0 = __int_as_float(max(__float_as_int(acc[e]), 0)) * mul;
  const float t1 = __int_as_float(max(__float_as_int(acc[8 + e]), 0)) * mul;
  amax = fmaxf(amax, fmaxf(t0, t1));
  const _Float16 a = (_Float16)t0, b = (_Float16)t1;
  hi0[e] = a;
  hi1[e] = b;
  if (PL == 2) {
    lo0[e] = (_Float16)(t0 - (float)a);
    lo1[e] = (_Float16)(t1 - (float)b);
  }
  asm volatile("" : "+v"(amax));      // keep the running maximum where it is computed (see dot_w4's pin in sdf_mlp_kernel.h)
}

template <int PL = 2, int G = 1, bool MIX = false>
__device__ __forceinline__ void split_tile(const f32x16& acc, const f32x16& accb, float mul, h8& hi0, h8& lo0, h8& hi1, h8& lo1, float& amax,
                                           int g = -1) {
#pragma unroll
  for (int e = 0; e < 8; ++e) split_part<PL, G, MIX>(acc, accb, mul, hi0, lo0, hi1, lo1, amax, e, g);
}

// a deferred tile epilogue is issued in kEpiChunks parts, one behind the MFMAs of each of the first K-blocks of a stage
constexpr int kEpiChunks = 8;
// ... starting at this K-block: the accumulator the epilogue reads was finished by the MFMA right in front of the stage,
// and an AGPR read within ~3 MFMAs of it waits for the matrix pipe (s_nop + dependency stall)
constexpr int kEpiShift = kS16Kb > 8 ? 1 : 0;
static_assert(kEpiShift + kEpiChunks <= kS16Kb, "epilogue slots");
struct NoOp16 {
  __device__ __forceinline__ void operator()(int, int = -1) const {}
};
typedef NoOp16 NoEpilogue16;

// make the compiler treat an accumulator as freshly defined here: element reads behind this statement cannot be hoisted
// in front of it (instruction selection otherwise copies a whole finished accumulator out of the AGPRs right behind its
// last MFMA - an s_nop 11 plus the wait for that MFMA at every tile boundary)
// (One-plane kernel with two point groups: the pin does the opposite there - with it the register allocator copies every finished
// layer-3 accumulator out of the AGPRs and back in, 64 moves and two s_nop 11 per tile: the one-plane kernels do not pin.)
template <int PL = 2>
__device__ __forceinline__ void pin_acc(f32x16& acc) {
  if (PL == 2) asm volatile("" : "+a"(acc));
}

// One LDS-DMA piece (1 KiB per wave) of the wave's share of a stage; P is the piece index.
// (Writing M0 once per four pieces instead of save / set / restore around each: -0.5 %, not worth relying on M0 surviving
// between asm statements.)
template <int P>
__device__ __forceinline__ void dma_piece(const float* src, unsigned dst) {
  lds_dma16_off<(P & 3) * 1024>(src + (P >> 2) * 1024, dst + (P >> 2) * 4096);
}

// K-block in front of which a stage's wait + barrier sit; the LDS-DMA pieces of the refill follow it
constexpr int kBarrierKb = kS16Kb / 2;
constexpr int kBarrierKbP1 = 12;      // ... of the one-plane kernel (16 KiB stages: the wait then covers pieces issued 2.75 stages ago)
// K-block of a tile's last stage whose region carries the next tile's preloads (biases / point fragments / w4: read half a tile ahead)
constexpr int kPreKb = kS16Kb / 2 + 2;

// One stage = kS16Kb K-blocks of one 32-row output tile: [kblock][plane hi / lo][lane][8 halves].
// On entry (ah[i], al[i]) hold the A fragments of K-blocks 0 .. PREFETCH-1 of THIS stage; on exit those of the next
// stage in stream order.  Every K-block is one scheduling region
//     [A-fragment reads of K-block kb + PREFETCH, pre(kb)]  fence  [3 MFMAs (+ DMA pieces), epi(kb)]  fence
// pre(kb) carries LDS reads whose results are wanted a K-block (or half a tile) later, epi(kb) the VALU work of the
// deferred epilogue.  The fence behind the reads is what keeps them AHEAD of the K-block's MFMAs: left to itself the
// scheduler sinks every LDS read to one MFMA (32 cycles) in front of its first use and the wave then sits in
// s_waitcnt for the rest of the LDS latency - 26 % of the wave cycles in the round-1 kernel (SQ_WAIT_ANY).
// ABL (timing only, tools/k1h_ablate.hip): 1 = no DMA / wait / barrier, 16 = no barrier,
// 32 = no DMA instructions (waits and barriers kept; the ring keeps the four stages loaded at the head start).
template <int KB, int Q, int SLOT, int ABL, int PL, int G, bool STEPS, class Pre, class Epi>
__device__ __forceinline__ void stage16(f32x16& acc, f32x16& accb, const h8 (&xh)[KB], const h8 (&xl)[KB], const float* ring,
                                        const float* next_src, unsigned lds_ring_base, int lane, int wave,
                                        h8 (&ah)[S16<PL, G>::kPrefetch], h8 (&al)[S16<PL, G>::kPrefetch], Pre&& pre, Epi&& epi) {
  constexpr int PF = S16<PL, G>::kPrefetch;
  constexpr int BKB = PL == 2 ? kBarrierKb : kBarrierKbP1;
  constexpr int nslot = (SLOT + kRing - 1) % kRing;   // slot of stage (this - 1), refilled with stage (this + 3)
  using SG = S16<PL, G>;
  const float* src = next_src + wave * SG::kWaveFloats + lane * 4;
  const unsigned dst = lds_ring_base + (nslot * SG::kFloats + wave * SG::kWaveFloats) * 4;
  const h8* cur = reinterpret_cast<const h8*>(ring + SLOT * SG::kFloats) + lane;
  const h8* nxt = reinterpret_cast<const h8*>(ring + ((SLOT + 1) % kRing) * SG::kFloats) + lane;
  h8 bufh[kS16Kb + PF], bufl[kS16Kb + PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) { bufh[i] = ah[i]; if (PL == 2) bufl[i] = al[i]; }
#pragma unroll
  for (int kb = 0; kb < kS16Kb; ++kb) {
    if (kb == BKB && !(ABL & 1)) {
      // my pieces of stage (this + 1) were issued 2.5 stages ago; only those of (this + 2) may stay in flight
      if (SG::kPieces == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      if (!(ABL & 16)) __builtin_amdgcn_s_barrier();
    }
    bufh[kb + PF] = kb + PF < kS16Kb ? cur[((kb + PF) * PL + 0) * 64] : nxt[((kb + PF - kS16Kb) * PL + 0) * 64];
    if (PL == 2) bufl[kb + PF] = kb + PF < kS16Kb ? cur[((kb + PF) * 2 + 1) * 64] : nxt[((kb + PF - kS16Kb) * 2 + 1) * 64];
    pre(kb);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int base = Q * kS16Kb;
#pragma unroll
    for (int j = 0; j < SG::kMfmas; ++j) {
      if (PL == 1 && j == 0) acc = ASDF_MFMA16(bufh[kb], xh[base + kb], acc);
      else if (PL == 1) accb = ASDF_MFMA16(bufh[kb], xl[base + kb], accb);       // the second point group, same A fragment
      else      // W_hi . x_lo, W_lo . x_hi, W_hi . x_hi - small terms first
        acc = ASDF_MFMA16(j == 1 ? bufl[kb] : bufh[kb], j == 0 ? xl[base + kb] : xh[base + kb], acc);
      // one DMA piece per MFMA shadow behind the barrier; split-half kernel (round 5): one per K-block, behind its LAST MFMA - the
      // gap that carries the least of a deferred epilogue part
      constexpr bool kDmaPerKb = STEPS && kS16Kb - BKB >= SG::kPieces;
      const int m = kDmaPerKb ? (j == 2 ? kb - BKB : -1) : (kb - BKB) * SG::kMfmas + j;
      if (!(ABL & 1) && !(ABL & 32) && m >= 0 && m < SG::kPieces) {
        if (m == 0) dma_piece<0>(src, dst);
        else if (m == 1) dma_piece<1>(src, dst);
        else if (m == 2) dma_piece<2>(src, dst);
        else if (m == 3) dma_piece<3>(src, dst);
        else if (m == 4) dma_piece<4>(src, dst);
        else if (m == 5) dma_piece<5>(src, dst);
        else if (m == 6) dma_piece<6>(src, dst);
        else dma_piece<7>(src, dst);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (PL == 1 && G == 2) {
        // two point groups: each group's share of the deferred epilogue goes behind ONE of the two MFMAs (left to itself the
        // scheduler issues both MFMAs back to back - the second waits a whole MFMA for the pipe - and then all the VALU work)
        epi(kb, j);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (STEPS) {
        // split-half kernel (round 5): the three pieces of a part behind the three MFMAs (split_part).  (The fence sits BEHIND the piece,
        // so a scheduling region is {MFMA j, piece j} and the scheduler puts the dependency-free piece in front of an MFMA that waits for
        // its LDS read now and then - every odd element: pieces 0 + 1 in one gap of 7 VALU instructions, still inside the MFMA's 32
        // clocks.  A fence on BOTH sides gives exactly 4 / 3 / 2 per gap, needs -pragma-unroll-threshold raised for the extra IR, and
        // measured the same: pipe busy 0.788 against 0.785 - not kept.)
        epi(kb, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (!((PL == 1 && G == 2) || STEPS)) epi(kb);
    // K-block = scheduling region (hoisted, 16 K-blocks of A fragments do not fit the register file either)
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < PF; ++i) { ah[i] = bufh[kS16Kb + i]; if (PL == 2) al[i] = bufl[kS16Kb + i]; }
}

// p.stream / p.cst are the split-half images here (pack_decoder_f16).  KP = K-steps of the point features on the fp32
// MFMA in layers 0 and 2: 2 = affine xyz, 5 / 8 = NeRF encoding of 9 / 15 features (those need 16 KiB stages: their
// constants block is 40 / 75 KiB).
// SUB: the kGridSubset form of sdf_mlp_kernel.h - the points are the lattice voxels listed in p.idx (p.count_dev of them, a
// device word; p.P is the list's capacity), coordinates from the voxel index, outputs scattered in place, no box.
template <bool TWO_OUT, int ABL = 0, int KP = 2, int PL = 2, int G = 1, bool SUB = false>
__device__ __forceinline__ void sdf_mlp_f16_body(const DecodeParams& p) {
  using CL = CstLayout<KP>;
  using SG = S16<PL, G>;
  static_assert(G == 1 || !TWO_OUT, "two point groups: SeparateDecoder");
  constexpr int kTilePts = kWgPts * G;           // points per workgroup tile
  // the plane split on v_fma_mix (split_part), issued in three pieces, one behind each MFMA of the part's K-block.  SeparateDecoder
  // forms only: the CombinedDecoder forms sit at the register limit with their second dot product - the asm blocks' simultaneous
  // destinations cost them 20 .. 48 B of scratch, and with the pieces their unrolled layer-3 loop exceeds the compiler's full-unroll
  // budget and comes out ROLLED, with indexed registers - and keep the round-2 form (same bits).
  constexpr bool kMix = PL == 2 && !TWO_OUT;
  constexpr bool kSteps = kMix;      // (the pieces exist only in the mix form of split_part)
  static_assert(lds_bytes_f16(KP, PL) <= 160 * 1024, "LDS budget");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;
  float* cst = smem + SG::kRingFloats;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;

  static_assert(!SUB || G == 1, "subset mode: one point group");
  // the lattice: by value, or - a fine pass enqueued behind its coarse pass - from the device words asdf_zoom_cube wrote
  float lat_vs = p.vs, lat_o0 = p.o0, lat_o1 = p.o1, lat_o2 = p.o2;
  if (p.lattice) { lat_o0 = p.lattice[0]; lat_o1 = p.lattice[1]; lat_o2 = p.lattice[2]; lat_vs = p.lattice[3]; }
  long long npts = p.P;
  if (SUB) { const long long c = *p.count_dev; npts = c < npts ? c : npts; }
  const long long ntiles = (npts + kTilePts - 1) / kTilePts;
  if ((long long)blockIdx.x >= ntiles) return;

  const unsigned lds_ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;
  // shader-clock stamps of workgroup 0 around a whole-lattice sweep (status words 12..13 begin, 14..15 end; s_memtime counts shader
  // clocks on gfx950): ticks / the launch's HIP-event time = the clock the part actually held under this kernel, which bench.py
  // reports next to the matrix-pipe utilisation.  Stored at once, so nothing stays live across the kernel.
  if (!SUB && p.status && p.mode != kPointList && blockIdx.x == 0 && tid == 0) reinterpret_cast<long long*>(p.status + ASDF_STATUS_CLOCK)[0] = clock64();

#pragma unroll 1
  for (int slot = 0; slot < p.num_mlps; ++slot) {
    const int head = p.first_mlp + slot;
    const float* hc = cst;
    // negative-voxel bounding box of this MLP's output(s) + the range report, one record per wave and output in LDS:
    // [0..2] min index, [3..5] max index, [6] count, [7] lanes whose activations left the fp16 range (or whose output is
    // not in [-1, 1]); the second output of a CombinedDecoder uses the record 8 ints further
    int* wrec = reinterpret_cast<int*>(cst + CL::kFloats) + wave * kWrecInts;
    // (empty_box_word written out: the call changes this kernel's ISA)
    if (lane < kWrecInts) wrec[lane] = lane >= 16 ? 0 : ((lane & 7) < 3 ? 0x7fffffff : ((lane & 7) < 6 ? -1 : 0));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(p.cst + (size_t)head * CL::kFloats);
      for (int i = tid; i < CL::kFloats / 4; i += 256) reinterpret_cast<f32x4*>(cst)[i] = src4[i];
    }
    // (one-plane kernels: the fp16 point-feature / bias operands of layers 0 and 2, behind the per-wave records)
    constexpr bool kPt16 = pt16(KP, PL);
    float* a16s = cst + CL::kFloats + kWaves * kWrecInts;
    if (kPt16) {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(p.a16 + (size_t)head * kA16Floats);
      for (int i = tid; i < kA16Floats / 4; i += 256)
        if (i < kA16LayerFloats / 4 || i >= 2 * kA16LayerFloats / 4) reinterpret_cast<f32x4*>(a16s)[i] = src4[i];      // (layer 2's operands are not used: see the tuning log)
    }
    const float* sbase0 = p.stream + (size_t)head * kS16Head * SG::kFloats;
#pragma unroll
    for (int s = 0; s < ((ABL & 33) ? kRing : kRing - 1); ++s) {
      const float* src = sbase0 + (size_t)s * SG::kFloats + wave * SG::kWaveFloats + lane * 4;
      const unsigned dst = lds_ring_base + (s * SG::kFloats + wave * SG::kWaveFloats) * 4;
#pragma unroll
      for (int c = 0; c < SG::kPieces; ++c) lds_dma16(src + c * 256, dst + c * 1024);
    }
    if (ABL & 33) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // my pieces of stage 0 (and my constants loads): those of stages 1 and 2 may stay in flight
    if (SG::kPieces == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __syncthreads();                                      // everybody's pieces of stage 0, and the constants
    h8 ah[SG::kPrefetch], al[SG::kPrefetch];
#pragma unroll
    for (int i = 0; i < SG::kPrefetch; ++i) {
      ah[i] = (reinterpret_cast<const h8*>(ring) + lane)[(i * PL + 0) * 64];
      if (PL == 2) al[i] = (reinterpret_cast<const h8*>(ring) + lane)[(i * 2 + 1) * 64];
    }
    // accumulator -> next layer's planes: S_x of the produced activations / (S_w S_x) of the accumulator (powers of two)
    const float mul1 = hc[CL::kB4 + 2], mul2 = hc[CL::kB4 + 3], mul0 = hc[CL::kB4 + 4];
    // subset mode: list positions from here on are audit picks (see DecodeParams::audit)
    int audit_from = 0x7fffffff;
    if (SUB && p.audit) audit_from = p.audit_from ? *p.audit_from : 0;

#pragma unroll 1
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const long long pi = tile * kTilePts + wave * (kWavePts * G) + (lane & 31);
      const bool valid = pi < npts;
      const long long po = SUB ? (valid ? (long long)p.idx[pi] : 0) : pi;      // where the point lives in the lattice / the outputs
      float x0 = 0.f, x1 = 0.f, x2 = 0.f;
      if (SUB) {
        grid_point(po, p.N, p.grid_mode, lat_vs, lat_o0, lat_o1, lat_o2, x0, x1, x2);
      } else if (p.mode == kPointList) {
        if (valid) { x0 = p.xyz[pi * 3 + 0]; x1 = p.xyz[pi * 3 + 1]; x2 = p.xyz[pi * 3 + 2]; }
      } else {
        grid_point(valid ? pi : 0, p.N, p.mode, lat_vs, lat_o0, lat_o1, lat_o2, x0, x1, x2);
      }
      // second point group (G == 2): the next 32 points
      const long long pib = pi + kWavePts;
      const bool validb = G == 2 && pib < npts;
      float bpb[KP];
#pragma unroll
      for (int s = 0; s < KP; ++s) bpb[s] = 0.0f;
      float y0 = 0.f, y1 = 0.f, y2 = 0.f;
      if (G == 2) {
        if (p.mode == kPointList) {
          if (validb) { y0 = p.xyz[pib * 3 + 0]; y1 = p.xyz[pib * 3 + 1]; y2 = p.xyz[pib * 3 + 2]; }
        } else {
          grid_point(validb ? pib : 0, p.N, p.mode, lat_vs, lat_o0, lat_o1, lat_o2, y0, y1, y2);
        }
        if (KP == 2) {
          bpb[0] = half ? y1 : y0;
          bpb[1] = half ? 0.0f : y2;
        } else {
#pragma unroll
          for (int s = 0; s < KP; ++s) bpb[s] = 2 * s + half < p.pf ? nerf_feature(2 * s + half, y0, y1, y2) : 0.0f;
        }
      }
      // largest plane value (x S_x) this lane hands to the fp16 conversion, per activation vector h0 / h1 / h2: >= 65504
      // is an overflow (range report); the maxima themselves go to the decoder's status record, from which the host
      // calibrates the S_x of each layer
      float amax = 0.0f, amax1 = 0.0f, amax2 = 0.0f;
      float bp[KP];
      if (KP == 2) {
        bp[0] = half ? x1 : x0;
        bp[1] = half ? 0.0f : x2;
      } else {
#pragma unroll
        for (int s = 0; s < KP; ++s) bp[s] = 2 * s + half < p.pf ? nerf_feature(2 * s + half, x0, x1, x2) : 0.0f;
      }
      // one-plane kernels: the points as the fp16 B operand of layers 0 / 2 (sdf_layout.h: kA16Floats) - x T in two planes, T twice
      // (the bias planes' multiplier) on lane half 0; the high planes again on lane half 1 (they meet the weights' low planes)
      auto point_operand = [&](float c0, float c1, float c2, float T) -> h8 {
        const float s0 = c0 * T, s1 = c1 * T, s2 = c2 * T;
        const _Float16 a0 = (_Float16)s0, a1 = (_Float16)s1, a2 = (_Float16)s2;
        h8 r;
        r[0] = a0; r[1] = a1; r[2] = a2;
        if (half == 0) {
          r[3] = (_Float16)(s0 - (float)a0); r[4] = (_Float16)(s1 - (float)a1); r[5] = (_Float16)(s2 - (float)a2);
          r[6] = (_Float16)T; r[7] = (_Float16)T;
        } else {
          r[3] = r[4] = r[5] = r[6] = r[7] = (_Float16)0.0f;
        }
        return r;
      };
      const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      h8 bq0, bq0b;
      if (kPt16) {
        bq0 = point_operand(x0, x1, x2, a16s[2 * kA16LayerFloats]);
        if (G == 2) bq0b = point_operand(y0, y1, y2, a16s[2 * kA16LayerFloats]);
      }
      auto a16_frag = [&](int layer, int t) -> h8 {      // this lane's 8 halves of tile t's operand
        return *reinterpret_cast<const h8*>(a16s + layer * kA16LayerFloats + t * kA16TileFloats + lane * 4);
      };
      const float* sbase = sbase0;
      asm volatile("" : "+s"(sbase));
      auto src_of = [&](int s) -> const float* {   // s = stage index within the head + 3
        return sbase + (size_t)(s < kS16Head ? s : s - kS16Head) * SG::kFloats;
      };

      // LDS reads that feed a tile are issued half a tile (or one K-block) ahead of their first use - `pre` slots of
      // stage16 - into registers that are dead at that point: the OTHER accumulator of the double buffer takes the next
      // tile's bias row, `pf2` its point-feature fragments, `w4n` the last-layer weights of the next epilogue part.
      f32x16 acc1[2], acc2[2], acc3[2];
      f32x16 acc1b[2], acc2b[2], acc3b[2];      // G == 2: the accumulators of the second point group
      float pf2[KP];                            // A fragments (fp32 MFMA) of the next layer-2 tile
      float w4c[2], w4n[2], w4bc[2], w4bn[2];   // last-layer weights of the current / next part of the layer-3 epilogue
      // one-plane kernel: all 16 of a tile's, read half a tile ahead (a K-block of 64 cycles is shorter than the LDS latency)
      constexpr bool kW4Tile = PL == 1 && !TWO_OUT;
      // layer 2 has ONE stage per tile: the preload of the next tile's bias row lands in the accumulator the deferred epilogue of
      // the previous tile is still reading until its last part (K-block kEpiShift + kEpiChunks - 1)
      static_assert(kS16Kb == 8 || kPreKb >= kEpiShift + kEpiChunks, "preload K-block inside the epilogue slots");
      f32x16 w4t;
      // (the 8 K-step form of PointFeatSize 15 has no registers to spare for these: it reads its fragments at the point of use)
      constexpr bool kPreloadPf = KP <= 5;
      auto load_pf2 = [&](int t) {
        if (!kPreloadPf) return;
#pragma unroll
        for (int s = 0; s < KP; ++s) pf2[s] = hc[CL::kA2 + (t * KP + s) * 64 + lane];
      };
      auto load_w4 = [&](int t, int c) {        // accumulator registers 2 c, 2 c + 1 of tile t
        const float* w4 = hc + CL::kW4 + (t * 2 + half) * 16 + 2 * c;
        const float* w4b = hc + CL::kW4b + (t * 2 + half) * 16 + 2 * c;
        w4n[0] = w4[0]; w4n[1] = w4[1];
        if (TWO_OUT) { w4bn[0] = w4b[0]; w4bn[1] = w4b[1]; }
      };
      auto next_w4 = [&]() {
        w4c[0] = w4n[0]; w4c[1] = w4n[1];
        if (TWO_OUT) { w4bc[0] = w4bn[0]; w4bc[1] = w4bn[1]; }
      };

      // ---- layer 0 (fp32 MFMA, K = 4 point features): planes of relu(.) * S_x
      h8 h0h[2 * kTilesHidden], h0l[2 * kTilesHidden];
      f32x16 acc0[2];
      float pf0[2][KP];
      auto l0_load = [&](int t) {
        if (!kPreloadPf) return;
        acc0[t & 1] = load_bias16(hc + CL::kC0 + (t * 2 + half) * 16);
#pragma unroll
        for (int s = 0; s < KP; ++s) pf0[t & 1][s] = hc[CL::kA0 + (t * KP + s) * 64 + lane];
      };
      auto l0_compute = [&](int t, int g = -1) {
        f32x16 acc = kPreloadPf ? acc0[t & 1] : load_bias16(hc + CL::kC0 + (t * 2 + half) * 16);
        f32x16 accb = acc;
#pragma unroll
        for (int s = 0; s < KP; ++s) {
          const float af = kPreloadPf ? pf0[t & 1][s] : hc[CL::kA0 + (t * KP + s) * 64 + lane];
          if (g != 1) acc = ASDF_MFMA(af, bp[s], acc);
          if (G == 2 && g != 0) accb = ASDF_MFMA(af, bpb[s], accb);
        }
        split_tile<PL, G, kMix>(acc, accb, mul0, h0h[2 * t], h0l[2 * t], h0h[2 * t + 1], h0l[2 * t + 1], amax, g);
      };
      // the split of a tile is ~100 VALU instructions against 128 cycles of fp32 MFMA: layer 0 is VALU-bound when it runs
      // on its own.  Only the tiles the first stage of layer 1 consumes (K-blocks 0 .. kS16Kb-1) are computed up front;
      // the others ride in the epilogue slots of that stage, under its fp16 MFMAs.
      constexpr int kL0Front = PL == 1 ? kTilesHidden : (kS16Kb / 2 < kEpiChunks ? kTilesHidden : kS16Kb / 2);
      if (PL == 1) {
        // One-plane kernel: all 16 tiles up front, software-pipelined over three accumulator sets - the bias / fragment reads
        // of tile t + 2, then the fp32 MFMAs of tile t + 1, then the fp16 conversions of tile t.  (Tile by tile, and with the
        // second half squeezed into the 64-cycle K-blocks of layer 1's first stage, layer 0 took 21.6 k of this kernel's
        // 124 k cycles per 256-point tile where its VALU work is 8 k: every tile waited for its LDS reads, then for its
        // MFMAs, then converted.)
        f32x16 la[3], lb[3];
        float lf[3][KP];
        h8 lq[3];
        auto l0p_load = [&](int t) {
          if (kPt16) { lq[t % 3] = a16_frag(0, t); return; }      // bias and point-feature columns in one fp16 operand
          la[t % 3] = load_bias16(hc + CL::kC0 + (t * 2 + half) * 16);
          if (G == 2) lb[t % 3] = load_bias16(hc + CL::kC0 + (t * 2 + half) * 16);
#pragma unroll
          for (int s = 0; s < KP; ++s) lf[t % 3][s] = hc[CL::kA0 + (t * KP + s) * 64 + lane];
        };
        auto l0p_mfma = [&](int t) {
          if (kPt16) {
            la[t % 3] = ASDF_MFMA16(lq[t % 3], bq0, zero16);
            if (G == 2) lb[t % 3] = ASDF_MFMA16(lq[t % 3], bq0b, zero16);
            return;
          }
#pragma unroll
          for (int s = 0; s < KP; ++s) {
            la[t % 3] = ASDF_MFMA(lf[t % 3][s], bp[s], la[t % 3]);
            if (G == 2) lb[t % 3] = ASDF_MFMA(lf[t % 3][s], bpb[s], lb[t % 3]);
          }
        };
        l0p_load(0);
        l0p_load(1);
        acc1[0] = load_bias16(hc + CL::kB1 + half * 16);
        if (G == 2) acc1b[0] = acc1[0];
        __builtin_amdgcn_sched_barrier(0);
        l0p_mfma(0);
#pragma unroll
        for (int t = 0; t < kTilesHidden; ++t) {
          if (t + 2 < kTilesHidden) l0p_load(t + 2);
          __builtin_amdgcn_sched_barrier(0);
          if (t + 1 < kTilesHidden) l0p_mfma(t + 1);
          split_tile<PL, G, kMix>(la[t % 3], lb[t % 3], mul0, h0h[2 * t], h0l[2 * t], h0h[2 * t + 1], h0l[2 * t + 1], amax);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
      l0_load(0);
      acc1[0] = load_bias16(hc + CL::kB1 + half * 16);
      if (G == 2) acc1b[0] = acc1[0];
#pragma unroll
      for (int t = 0; t < kL0Front; ++t) {
        if (t + 1 < kTilesHidden) { l0_load(t + 1); __builtin_amdgcn_sched_barrier(0); }
        l0_compute(t);
        __builtin_amdgcn_sched_barrier(0);
      }
      }

#define ASDF_STAGE16(KB, Q, SLOT, ACC, XH, XL, SIDX, PRE, EPI) \
  stage16<KB, Q, SLOT, ABL, PL, G, kSteps>(ACC, ACC##b, XH, XL, ring, src_of((SIDX) + 3), lds_ring_base, lane, wave, ah, al, PRE, EPI)

      // (split-half kernel: the second argument of an epilogue callback is the PIECE of the part - stage16 calls it behind each of
      // the K-block's three MFMAs - and `er` carries a part's two ReLUs from piece to piece)
      float er[2] = {0.0f, 0.0f};
      // ---- layer 1: 512 -> 256; epilogue of tile t-1 rides in tile t
      h8 h1h[2 * kTilesL1], h1l[2 * kTilesL1];
      if (ABL & 4) for (int t = 0; t < 2 * kTilesL1; ++t) { h1h[t] = h0h[t]; h1l[t] = h0l[t]; }
#pragma unroll
      for (int t = 0; t < kTilesL1; ++t) {
        f32x16& acc = acc1[t & 1];
        f32x16& accb = (G == 2 ? acc1b : acc1)[t & 1];
        auto pre = [&](int kb) {       // first stage: the layer-0 tile of the NEXT K-block's epilogue slot
          const int c = kb - kEpiShift;
          if (t == 0 && kL0Front < kTilesHidden && c >= 0 && c + 1 < kEpiChunks) l0_load(kL0Front + c + 1);
        };
        auto epi = [&](int kb, int g = -1) {
          const int c = kb - kEpiShift;
          if (c < 0 || c >= kEpiChunks) return;
          if (t == 0) {
            if (kSteps && kPreloadPf && kL0Front < kTilesHidden) {
              // a whole layer-0 tile per K-block: its fp32 MFMAs behind the first MFMA, its eight parts over the three gaps (3 + 3 + 2)
              const int T = kL0Front + c;
              if (g == 0) {
#pragma unroll
                for (int s = 0; s < KP; ++s) acc0[T & 1] = ASDF_MFMA(pf0[T & 1][s], bp[s], acc0[T & 1]);
              }
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if (e / 3 == g) split_part<PL, G, kMix>(acc0[T & 1], acc0[T & 1], mul0, h0h[2 * T], h0l[2 * T], h0h[2 * T + 1], h0l[2 * T + 1], amax, e);
              return;
            }
            if (kSteps && g > 0) return;
            if (kL0Front < kTilesHidden) l0_compute(kL0Front + c, kSteps ? -1 : g);       // layer-0 tiles 8 .. 15: consumed by the next stage
            return;
          }
          if (ABL & 4) { asm volatile("" :: "v"(acc1[(t - 1) & 1])); return; }
          if (kSteps ? g <= 0 : g != 1) pin_acc<PL>(acc1[(t - 1) & 1]);
          if (G == 2 && g != 0) pin_acc<PL>(acc1b[(t - 1) & 1]);
          split_part<PL, G, kMix>(acc1[(t - 1) & 1], acc1b[(t - 1) & 1], mul1, h1h[2 * (t - 1)], h1l[2 * (t - 1)], h1h[2 * (t - 1) + 1],
                            h1l[2 * (t - 1) + 1], amax1, c, kSteps ? -1 : g, kSteps ? g : -1, er);
        };
        auto pre_last = [&](int c) {   // last stage: bias row (and point fragments) of the next tile
          if (c != kPreKb) return;
          if (t + 1 < kTilesL1) { acc1[(t + 1) & 1] = load_bias16(hc + CL::kB1 + ((t + 1) * 2 + half) * 16); if (G == 2) acc1b[(t + 1) & 1] = acc1[(t + 1) & 1]; }
          else { acc2[0] = load_bias16(hc + CL::kC2 + half * 16); if (G == 2) acc2b[0] = acc2[0]; load_pf2(0); }
        };
#if ASDF16_STAGE_KB == 8
        ASDF_STAGE16(32, 0, 0, acc, h0h, h0l, t * 4 + 0, pre, epi);
        ASDF_STAGE16(32, 1, 1, acc, h0h, h0l, t * 4 + 1, NoOp16(), NoOp16());
        ASDF_STAGE16(32, 2, 2, acc, h0h, h0l, t * 4 + 2, NoOp16(), NoOp16());
        ASDF_STAGE16(32, 3, 3, acc, h0h, h0l, t * 4 + 3, pre_last, NoOp16());
#else
        if (t & 1) {
          ASDF_STAGE16(32, 0, 2, acc, h0h, h0l, t * 2 + 0, pre, epi);
          ASDF_STAGE16(32, 1, 3, acc, h0h, h0l, t * 2 + 1, pre_last, NoOp16());
        } else {
          ASDF_STAGE16(32, 0, 0, acc, h0h, h0l, t * 2 + 0, pre, epi);
          ASDF_STAGE16(32, 1, 1, acc, h0h, h0l, t * 2 + 1, pre_last, NoOp16());
        }
#endif
      }

      // ---- layer 2: [h1 (256) | xyz (4, fp32 MFMA, pre-scaled A fragments)] -> 512
      h8 h2h[2 * kTilesHidden], h2l[2 * kTilesHidden];
      if (ABL & 4) for (int t = 0; t < 2 * kTilesHidden; ++t) { h2h[t] = h0h[t]; h2l[t] = h0l[t]; }
      // one tile of layer 2; SLOT is the ring slot of its first stage (a tag type: the slot must be a compile-time constant)
      auto l2_tile = [&](int t, auto slot_tag) {
        constexpr int SLOT = decltype(slot_tag)::value;
        f32x16& acc = acc2[t & 1];
        f32x16& accb = (G == 2 ? acc2b : acc2)[t & 1];
#pragma unroll
        for (int s = 0; s < KP; ++s) {
          const float af = kPreloadPf ? pf2[s] : hc[CL::kA2 + (t * KP + s) * 64 + lane];
          acc = ASDF_MFMA(af, bp[s], acc);
          if (G == 2) accb = ASDF_MFMA(af, bpb[s], accb);
        }
        auto epi = [&](int kb, int g = -1) {
          const int c = kb - kEpiShift;
          if (c < 0 || c >= kEpiChunks) return;
          if (ABL & 4) { asm volatile("" :: "v"(acc2[(t + 1) & 1]), "v"(acc1[1])); return; }
          if (t > 0) {
            if (kSteps ? g <= 0 : g != 1) pin_acc<PL>(acc2[(t - 1) & 1]);
            if (G == 2 && g != 0) pin_acc<PL>(acc2b[(t - 1) & 1]);
            split_part<PL, G, kMix>(acc2[(t - 1) & 1], acc2b[(t - 1) & 1], mul2, h2h[2 * (t - 1)], h2l[2 * (t - 1)], h2h[2 * (t - 1) + 1],
                              h2l[2 * (t - 1) + 1], amax2, c, kSteps ? -1 : g, kSteps ? g : -1, er);
          } else {
            if (kSteps ? g <= 0 : g != 1) pin_acc<PL>(acc1[(kTilesL1 - 1) & 1]);
            if (G == 2 && g != 0) pin_acc<PL>(acc1b[(kTilesL1 - 1) & 1]);
            split_part<PL, G, kMix>(acc1[(kTilesL1 - 1) & 1], acc1b[(kTilesL1 - 1) & 1], mul1, h1h[2 * kTilesL1 - 2], h1l[2 * kTilesL1 - 2],
                              h1h[2 * kTilesL1 - 1], h1l[2 * kTilesL1 - 1], amax1, c, kSteps ? -1 : g, kSteps ? g : -1, er);      // K-blocks 14, 15: consumed at the end of this tile, after chunk 7
          }
        };
        auto pre_last = [&](int c) {
          if (c != kPreKb) return;
          if (t + 1 < kTilesHidden) {
            acc2[(t + 1) & 1] = load_bias16(hc + CL::kC2 + ((t + 1) * 2 + half) * 16);
            if (G == 2) acc2b[(t + 1) & 1] = acc2[(t + 1) & 1];
            load_pf2(t + 1);
          } else {
            acc3[0] = load_bias16(hc + CL::kB3 + half * 16);
            if (G == 2) acc3b[0] = acc3[0];
          }
        };
        constexpr int S0 = 256 / kS16Kb;         // stages of layer 1
#if ASDF16_STAGE_KB == 8
        ASDF_STAGE16(16, 0, SLOT, acc, h1h, h1l, S0 + t * 2 + 0, NoOp16(), epi);
        ASDF_STAGE16(16, 1, SLOT + 1, acc, h1h, h1l, S0 + t * 2 + 1, pre_last, NoOp16());
#else
        ASDF_STAGE16(16, 0, SLOT, acc, h1h, h1l, S0 + t, pre_last, epi);      // one stage per tile
#endif
      };
#pragma unroll
      for (int tt = 0; tt < kTilesHidden / 4; ++tt) {
#if ASDF16_STAGE_KB == 8
        l2_tile(4 * tt + 0, std::integral_constant<int, 0>());
        l2_tile(4 * tt + 1, std::integral_constant<int, 2>());
        l2_tile(4 * tt + 2, std::integral_constant<int, 0>());
        l2_tile(4 * tt + 3, std::integral_constant<int, 2>());
#else
        l2_tile(4 * tt + 0, std::integral_constant<int, 0>());
        l2_tile(4 * tt + 1, std::integral_constant<int, 1>());
        l2_tile(4 * tt + 2, std::integral_constant<int, 2>());
        l2_tile(4 * tt + 3, std::integral_constant<int, 3>());
#endif
      }

      // ---- layer 3 (512 -> 512) fused with layer 4 (dot with w4 / (S_w3 S_x)) and tanh
      float part = 0.0f, partb = 0.0f, partg = 0.0f;      // partg: the second point group's dot product (G == 2)
      // accumulator registers 2 c, 2 c + 1 of a finished tile into the last-layer dot product(s), weights from (w4c, w4bc)
      auto dot_w4_part = [&](const f32x16& a, const f32x16& ab, int c, int g = -1, int only = -1) {      // only: 0 / 1 = that register of the pair
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (only >= 0 && only != r) continue;
          const float w = kW4Tile ? w4t[2 * c + r] : w4c[r];
          if (PL == 1) {
            // relu(a) w = a (w / 2) + |a| (w / 2): two FMAs like max + FMA, and a NaN / infinity of either sign stays one (the image's
            // last-layer weights carry the 1 / 2)
            if (g != 1) {
              const float v = a[2 * c + r];
              part = fmaf(fabsf(v), w, fmaf(v, w, part));
              if (TWO_OUT) partb = fmaf(fabsf(v), w4bc[r], fmaf(v, w4bc[r], partb));
            }
            if (G == 2 && g != 0) { const float v = ab[2 * c + r]; partg = fmaf(fabsf(v), w, fmaf(v, w, partg)); }
            continue;
          }
          if (g != 1) {
            const float v = __int_as_float(max(__float_as_int(a[2 * c + r]), 0));
            part = fmaf(v, w, part);
            if (TWO_OUT) partb = fmaf(v, w4bc[r], partb);
          }
          if (G == 2 && g != 0) partg = fmaf(__int_as_float(max(__float_as_int(ab[2 * c + r]), 0)), w, partg);
        }
        if (TWO_OUT) asm volatile("" : "+v"(part), "+v"(partb));
        if (G == 2) asm volatile("" : "+v"(part), "+v"(partg));
      };
#pragma unroll
      for (int t = 0; t < kTilesHidden; ++t) {
        f32x16& acc = acc3[t & 1];
        f32x16& accb = (G == 2 ? acc3b : acc3)[t & 1];
        auto pre = [&](int kb) {       // first stage: w4 of the next epilogue part
          const int c = kb - kEpiShift;
          if (!kW4Tile && t > 0 && c >= 0 && c + 1 < kEpiChunks) load_w4(t - 1, c + 1);
        };
        auto epi = [&](int kb, int g = -1) {
          const int c = kb - kEpiShift;
          if (c < 0 || c >= kEpiChunks) return;
          if (ABL & 4) { asm volatile("" :: "v"(acc3[(t + 1) & 1]), "v"(acc2[1])); return; }
          if (t > 0) {
            if (kSteps ? g <= 0 : g != 1) pin_acc<PL>(acc3[(t - 1) & 1]);
            if (G == 2 && g != 0) pin_acc<PL>(acc3b[(t - 1) & 1]);
            if (kSteps) {        // piece 0 / 1: one register of the pair each; piece 2: the next pair's weights
              if (g < 2) dot_w4_part(acc3[(t - 1) & 1], acc3b[(t - 1) & 1], c, -1, g);
              if (!kW4Tile && (g == 2 || g < 0)) next_w4();
            } else {
              dot_w4_part(acc3[(t - 1) & 1], acc3b[(t - 1) & 1], c, g, -1);
              if (!kW4Tile && g != 0) next_w4();            // (both groups use the same weights: rotate behind the second)
            }
          } else {
            if (kSteps ? g <= 0 : g != 1) pin_acc<PL>(acc2[(kTilesHidden - 1) & 1]);
            if (G == 2 && g != 0) pin_acc<PL>(acc2b[(kTilesHidden - 1) & 1]);
            split_part<PL, G, kMix>(acc2[(kTilesHidden - 1) & 1], acc2b[(kTilesHidden - 1) & 1], mul2, h2h[2 * kTilesHidden - 2],
                              h2l[2 * kTilesHidden - 2], h2h[2 * kTilesHidden - 1], h2l[2 * kTilesHidden - 1], amax2, c, kSteps ? -1 : g,
                              kSteps ? g : -1, er);  // K-blocks 30, 31: end of this tile
          }
        };
        auto pre_last = [&](int c) {   // last stage: bias row of the next tile, w4 of the first part of this tile's epilogue
          if (c != kPreKb) return;
          if (t + 1 < kTilesHidden) {
            acc3[(t + 1) & 1] = load_bias16(hc + CL::kB3 + ((t + 1) * 2 + half) * 16);
            if (G == 2) acc3b[(t + 1) & 1] = acc3[(t + 1) & 1];
          }
          if (kW4Tile) { w4t = load_bias16(hc + CL::kW4 + (t * 2 + half) * 16); return; }
          load_w4(t, 0);
          next_w4();
        };
        constexpr int S0 = 512 / kS16Kb;         // stages of layers 1 and 2
#if ASDF16_STAGE_KB == 8
        ASDF_STAGE16(32, 0, 0, acc, h2h, h2l, S0 + t * 4 + 0, pre, epi);
        ASDF_STAGE16(32, 1, 1, acc, h2h, h2l, S0 + t * 4 + 1, NoOp16(), NoOp16());
        ASDF_STAGE16(32, 2, 2, acc, h2h, h2l, S0 + t * 4 + 2, NoOp16(), NoOp16());
        ASDF_STAGE16(32, 3, 3, acc, h2h, h2l, S0 + t * 4 + 3, pre_last, NoOp16());
#else
        if (t & 1) {
          ASDF_STAGE16(32, 0, 2, acc, h2h, h2l, S0 + t * 2 + 0, pre, epi);
          ASDF_STAGE16(32, 1, 3, acc, h2h, h2l, S0 + t * 2 + 1, pre_last, NoOp16());
        } else {
          ASDF_STAGE16(32, 0, 0, acc, h2h, h2l, S0 + t * 2 + 0, pre, epi);
          ASDF_STAGE16(32, 1, 1, acc, h2h, h2l, S0 + t * 2 + 1, pre_last, NoOp16());
        }
#endif
      }
      // the last tile's epilogue has no MFMA stream to hide under
#pragma unroll
      for (int c = 0; c < kEpiChunks; ++c) {
        if (!kW4Tile && c + 1 < kEpiChunks) load_w4(kTilesHidden - 1, c + 1);
        dot_w4_part(acc3[(kTilesHidden - 1) & 1], acc3b[(kTilesHidden - 1) & 1], c);
        if (!kW4Tile) next_w4();
      }
#undef ASDF_STAGE16
      auto tanh_out = [&](float x) -> float {
        // one plane: 1 - 2 / (1 + exp(2 x)) on the hardware exp / rcp (absolute error ~1e-7; the values carry ~1e-4)
        if (PL == 1) return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
        return tanhf(x);
      };
      part += __shfl_xor(part, 32);
      const float pre = part + hc[CL::kB4];           // (pre-activations: the strict range report below looks at THESE)
      const float sdf = tanh_out(pre);
      float sdfb = 1.0f, preb = 0.0f, preg = 0.0f;
      if (TWO_OUT) {
        partb += __shfl_xor(partb, 32);
        preb = partb + hc[CL::kB4 + 1];
        sdfb = tanh_out(preb);
      }
      float sdfg = 0.0f;           // the second point group's output (G == 2)
      if (G == 2) {
        partg += __shfl_xor(partg, 32);
        preg = partg + hc[CL::kB4];
        sdfg = tanh_out(preg);
      }
      const bool is_hand = head == 0;
      if (SUB) {
        // subset mode replaces values: the largest change is the measured error of the arithmetic it corrects.  Marked voxels
        // report to ASDF_STATUS_MAX_ERR; audit picks (voxels the one-plane sweep decided by sign alone) to the audit record, together
        // with the number of picks whose sign the exact value contradicts.  Reduced over the wave on the float BITS (a NaN
        // is a huge pattern and must survive the reduction), then one set of atomics per wave.
        int dm = 0, da = 0, flips = 0, na = 0;
        float sq = 0.0f;           // sum of squared audit errors: sigma of the one-plane error, next to its maximum
        if (valid && half == 0) {
          const bool aud = p.audit && pi >= (long long)audit_from;
          auto replace = [&](float* vol, float now) {
            const float before = vol[po];
            const int d = __float_as_int(fabsf(now - before));
            if (aud) { da = max(da, d); flips += ((before < 0.0f) != (now < 0.0f)) ? 1 : 0; ++na; sq += (now - before) * (now - before); }
            else dm = max(dm, d);
            // (a list of audit picks alone - the box sweep's - leaves the scratch volume as the one-plane kernel wrote it: that audit
            // runs BESIDE the collection of the sweep's candidates, which reads the same volume; round 5)
            if (!aud || p.audit_from) vol[po] = now;
          };
          float* out = is_hand ? p.sdf0 : p.sdf1;
          if (out) replace(out, sdf);
          if (TWO_OUT && p.sdf1) replace(p.sdf1, sdfb);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          dm = max(dm, __shfl_xor(dm, m)); da = max(da, __shfl_xor(da, m));
          flips += __shfl_xor(flips, m); na += __shfl_xor(na, m);
          if (p.audit) sq += __shfl_xor(sq, m);
        }
        if (lane == 0) {
          if (p.status && dm) atomicMax(p.status + ASDF_STATUS_MAX_ERR, dm);
          if (p.audit && na) {
            atomicMax(p.audit + kAuditMaxErr, da); if (flips) atomicAdd(p.audit + kAuditFlips, flips); atomicAdd(p.audit + kAuditEvals, na);
            atomicAdd(reinterpret_cast<float*>(p.audit + kAuditSumSq), sq);
          }
        }
      } else if (valid && half == 0) {
        float* out = is_hand ? p.sdf0 : p.sdf1;
        if (out) out[po] = sdf;
        if (TWO_OUT && p.sdf1) p.sdf1[po] = sdfb;
      }
      if (G == 2 && validb && half == 1) {       // lanes 32..63 store the second group: 64 consecutive floats per wave
        float* out = is_hand ? p.sdf0 : p.sdf1;
        if (out) out[pib] = sdfg;
      }
      // every lane reports its own activations (the two halves of a wave hold different features of the same point):
      // a lane is out of range when a value handed to the fp16 conversion reached 65504 (|x| >= 8188) or an output left
      // [-1, 1] (NaN / infinity downstream of an overflow).  The count goes to the decoder's status word - always, not only
      // when the caller passed a bbox buffer - and, for grid sweeps with a bbox, to word 7 / 15 of that record as well.
      // (one-plane kernels, folded image: no running maximum - every ReLU preserves a poisoned value, so an activation that left the
      // fp16 range arrives HERE as a non-finite PRE-activation of the tanh: a NaN, or an infinity.  The check is on that value, not
      // on the output - tanhf returns exactly +-1 for every finite argument beyond ~9, so a decoder that merely saturates in the far
      // field must not read as a range violation: ADVICE r04, it drove such a decoder through four re-calibrations to the fp32 chain)
      constexpr bool kStrict = PL == 1;
      if (kMix) { amax *= mul0; amax1 *= mul1; amax2 *= mul2; }      // (the maxima were taken in front of the rescale)
      const bool act_over = !(fmaxf(amax, fmaxf(amax1, amax2)) < 65504.0f);
      auto out_ok = [&](float v, float pre_v) { return kStrict ? fabsf(pre_v) < INFINITY : fabsf(v) <= 1.0f; };
      const int bad = ((valid || validb) && (act_over || !out_ok(sdf, pre) || (TWO_OUT && !out_ok(sdfb, preb)) ||
                                            (G == 2 && !out_ok(sdfg, preg)))) ? 1 : 0;
      if (!kStrict && p.status) {
        // per-wave peaks of the three activation vectors: non-negative floats order like their bit patterns, a NaN is a huge
        // pattern and reads as overflow.  One DPP reduction per value and a plain read-modify-write by one lane (the record is the
        // wave's own).  Round 5: this was three LDS atomicMax by all 64 lanes on ONE word each - 14 k clocks per tile, a tenth of
        // the kernel, and only in the product (the timing tool passed no status record: tools/k1h_ablate.hip K1H_STATUS=1).
        const bool v_ = valid || validb;
        const int m0 = wave_max_i32(v_ ? __float_as_int(amax) : 0), m1 = wave_max_i32(v_ ? __float_as_int(amax1) : 0),
                  m2 = wave_max_i32(v_ ? __float_as_int(amax2) : 0);
        if (lane == 0) { wrec[16] = max(wrec[16], m0); wrec[17] = max(wrec[17], m1); wrec[18] = max(wrec[18], m2); }
      }
      if (!SUB && p.bbox && p.mode != kPointList) {
        // with two point groups every lane folds ITS point: lanes 0..31 the first group's, lanes 32..63 the second's
        const long long pf_ = (G == 2 && half == 1) ? pib : pi;
        auto fold = [&](bool neg, int* rec, int extra) {
          if ((PL == 1 || kMix) && !__any(neg || extra != 0)) return;      // (wave-uniform: most tiles of a sweep hold no negative voxel; round 5: the split-half SeparateDecoder forms too)
          int i0, i1, i2;                                        // (behind the early return: two integer divisions per lane)
          lattice_ijk(pf_, p.N, i0, i1, i2);
          int a0 = neg ? i0 : 0x7fffffff, a1 = neg ? i1 : 0x7fffffff, a2 = neg ? i2 : 0x7fffffff;
          int b0 = neg ? i0 : -1, b1 = neg ? i1 : -1, b2 = neg ? i2 : -1, n = neg ? 1 : 0;
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) {
            a0 = min(a0, __shfl_xor(a0, m)); a1 = min(a1, __shfl_xor(a1, m)); a2 = min(a2, __shfl_xor(a2, m));
            b0 = max(b0, __shfl_xor(b0, m)); b1 = max(b1, __shfl_xor(b1, m)); b2 = max(b2, __shfl_xor(b2, m));
            n += __shfl_xor(n, m);
            extra += __shfl_xor(extra, m);
          }
          if (lane == 0 && (n | extra)) {
            rec[0] = min(rec[0], a0); rec[1] = min(rec[1], a1); rec[2] = min(rec[2], a2);
            rec[3] = max(rec[3], b0); rec[4] = max(rec[4], b1); rec[5] = max(rec[5], b2);
            rec[6] += n; rec[7] += extra;
          }
        };
        if (G == 2) fold(half == 0 ? (valid && sdf < p.neg_thr) : (validb && sdfg < p.neg_thr), wrec, bad);
        else fold(valid && half == 0 && sdf < p.neg_thr, wrec, bad);
        if (TWO_OUT) fold(valid && half == 0 && sdfb < p.neg_thr, wrec + 8, 0);
      } else {
        const unsigned long long m = __ballot(bad);
        if (m && lane == 0) wrec[7] += __popcll(m);
      }
    }   // tiles

    if (lane == 0) {
      // one set of atomics per wave: record 0 = hand (MLP 0 / first row), record 1 = object (MLP 1 / second row);
      // word 7: lanes out of range (0 unless the fp16 planes overflowed; the host then falls back to fp32)
      auto flush = [&](int* out, const int* rec) {
        if (rec[6]) {      // (not flush_box: reading the LDS record up front instead of word by word changes this kernel's ISA)
          atomicMin(out + ASDF_BOX_MIN + 0, rec[0]); atomicMin(out + ASDF_BOX_MIN + 1, rec[1]); atomicMin(out + ASDF_BOX_MIN + 2, rec[2]);
          atomicMax(out + ASDF_BOX_MAX + 0, rec[3]); atomicMax(out + ASDF_BOX_MAX + 1, rec[4]); atomicMax(out + ASDF_BOX_MAX + 2, rec[5]);
          atomicAdd(out + ASDF_BOX_COUNT, rec[6]);
        }
      };
      if (p.bbox && p.mode != kPointList) {
        flush(p.bbox + (head == 0 ? 0 : ASDF_BOX_STRIDE), wrec);
        if (TWO_OUT) flush(p.bbox + ASDF_BOX_STRIDE, wrec + 8);
        if (wrec[7]) atomicAdd(p.bbox + (head == 0 ? ASDF_BOX_RANGE : ASDF_BOX_STRIDE + ASDF_BOX_RANGE), wrec[7]);
      }
      if (p.status) {
        if (wrec[7]) atomicAdd(p.status + ASDF_STATUS_RANGE, wrec[7]);
        int* peak = p.status + ASDF_STATUS_PEAK + ASDF_STATUS_PEAK_STRIDE * head;       // largest plane value of h0 / h1 / h2 (float bits)
        atomicMax(peak + 0, wrec[16]); atomicMax(peak + 1, wrec[17]); atomicMax(peak + 2, wrec[18]);
      }
    }
  }   // MLPs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!SUB && p.status && p.mode != kPointList && blockIdx.x == 0 && tid == 0) reinterpret_cast<long long*>(p.status + ASDF_STATUS_CLOCK)[1] = clock64();
}

// The __global__ instantiations live in k1h_kernels.hip; tools/k1h_ablate.hip instantiates its own.

}  // namespace asdf
