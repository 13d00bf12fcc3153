// Host side of the decoder C ABI (include/alignsdf_hip.h): the decoder object, weight packing and the host flow of the sweeps -
// the launches of the fused MLP kernels (K1, k1_launch.h) and of the small kernels around them (fold_kernels.h, sweep_kernels.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/alignsdf_hip.h"
#include "common.h"
#include "pack.h"
#include "k1_launch.h"
#include "fold_kernels.h"
#include "sweep_kernels.h"

namespace asdf {
thread_local int g_last_hip_error = 0;
}

using namespace asdf;

struct asdf_decoder {
  asdf_decoder_spec_t spec;
  int device;
  int num_cus;
  float* stream;    // [kStagesAll][kStageFloats]
  float* wlat;      // [heads][2][512][256]
  float* wpt;       // [heads][2][512][MAXPF]
  float* bias02;    // [heads][2][512]
  float* cst;       // [heads][cst_offsets(kp).floats]  (static parts written at create time)
  int kp;           // point-feature K-steps: 2 (affine xyz) or ceil(pf / 2) (NeRF encoding)
  float* embed;     // [heads][MAXPF][4]
  float* latent_stage;   // [kLatent]: the latent of a sample whose codes came from host memory (asdf_decoder_set_sample_host)
  float* cls;       // [kMaxClasses][512 in D-layout order] + [kMaxClasses]; null until asdf_decoder_set_classifier
  int num_class;
  // split-half image (pack_decoder_f16) and the arithmetic in use
  float* stream16;
  float* stream16_hi;   // the high planes alone (1 KiB records): weight stream of the one-plane kernel (asdf_decode_grid_box)
  float* cst16;
  float* a16;       // [heads][kA16Floats] fp16 point-feature / bias operands of the one-plane kernels (K0b, per sample; affine features only)
  // The one-plane kernels' OWN image (round 4): weight scales chosen so that every accumulator already carries its activation's
  // plane scale - S_w1' = S_x1 / S_x0, S_w2' = S_x2 / S_x1, layer 0's constants times S_x0 - and the epilogue needs no rescale
  // (a v_pk_mul_f32 per register pair: with the range maximum, a third of the kernel's VALU issue).  cst16p1 = its constants
  // block, stream16_hi's layer-1 / layer-2 records = the high planes times S_w' / S_w (exact: powers of two); both are rebuilt
  // from the host copies whenever the activation scales change.
  float* cst16p1;
  float* cst16p1_host;
  uint16_t* hi_host;      // high planes at the split-half scales (the base of every rebuild), hi_count halves
  uint16_t* hi_scaled;    // staging buffer of the rescaled image
  size_t hi_count;
  float s0p[ASDF_MAX_HEADS], s2p[ASDF_MAX_HEADS];
  int p1_usable;          // 0: a rescaled weight would leave the fp16 range - the one-plane sweeps are not offered for this decoder
  float s2[ASDF_MAX_HEADS];
  int math;
  bool sample_bound;
  int* status;      // [ASDF_STATUS_WORDS] device words: the status record (include/alignsdf_hip.h: ASDF_STATUS_*)
  // activation scales of the split-half image (asdf_decoder_set_act_scales) and what is needed to rebuild its constants
  float sw[ASDF_MAX_HEADS][3];
  float sx[ASDF_MAX_HEADS][3];
  float* cst_host;    // the fp32 constants image (static parts), host copy
  float* cst16_host;  // staging buffer of the rebuilt split-half constants
  // near-level refinement of split-half sweeps (asdf_decoder_set_refine)
  void* ev_start;   // one-shot hipEvent_t pair recorded around the dominant kernel of the next sweep (asdf_decoder_time_next_sweep)
  void* ev_stop;
  float refine_tau;
  int* near_idx;    // [kNearCap] lattice indices
  int* near_count;  // device word
  // narrow-band fine sweep (asdf_decode_grid_band): voxel marks and the per-head re-evaluation lists, allocated on first use
  unsigned char* band_mark;
  size_t band_mark_bytes;
  int* box_aux;     // box-only sweep, large candidate lists: [0..2] count words, [4 ..] near-level voxels among the candidates (kNearCap)
  int* band_idx;    // [2][kBandCap]
  int* band_count;  // [2] device words
  // the exact re-evaluation of a short voxel list is latency-bound (one 128-point tile of one MLP on the fp32 chain takes
  // 0.24 ms whatever the list holds): the two MLPs of a SeparateDecoder run side by side, the second on this stream
  hipStream_t side;
  hipEvent_t ev_fork, ev_join;
  // audit of the one-plane sweeps (asdf_decoder_set_audit): voxels per sweep and head, the seed of the next draw, the record
  // (sweep_records.h: AuditWord), and the voxel list of the box sweep's audit
  int audit_n;
  unsigned long long audit_seed;
  int* audit_rec;   // [kAuditWords]
  int* audit_idx;   // [kAuditCap]
  int* audit_count;
  int short_max;    // voxel lists of up to this many points are re-evaluated by the short-list form of the fp32 chain (0 = never)
  // ... and the shortest ones by its cluster form (four workgroups per 32 points): exchange buffers and arrival counters of
  // kShortClusters clusters (asdf_decoder_set_cluster_list)
  ShortParams shortp;
  // the audit of a box sweep runs beside the exact re-evaluation of its candidates (round 5)
  hipStream_t audit_side;
  hipEvent_t ev_audit_fork, ev_audit_join;
  // pixel-aligned latent (asdf_decoder_set_sample_pixel): bound instead of a latent code until the next asdf_decoder_set_sample*
  bool pixel_bound;
  PixelParams pixel;      // the per-sample scalars and the buffers below, as the kernel reads them
  float* pa_proj;         // [heads][2][H W][512]: P = W_lat . F, grown on demand (32 MiB at 64 x 64)
  size_t pa_proj_floats;
  float* pa_cstb;         // [heads][cst floats]: the constants image folded with a zero latent (its c0 / c2 blocks = the biases)
  float* pa_ws;           // [num_cus][kPixelWsFloats] workspace of the pixel-aligned kernel
  float* pa_lat;          // [2][kLatent]: the channel mean of F, zeros
  unsigned long long* trace_queue;   // [2] device words: the per-head ray queues of asdf_trace_rays (cleared in stream order per call)
  // reverse mode (asdf_decode_points_vjp): the transposed weight image (null for decoders the form does not cover) and, allocated on
  // first use, the workgroups' partial sums [num_cus][kVjpFoldFloats] followed by one d_fold block for callers that pass none
  float* streamT;
  float* vjp_partial;
};
static constexpr int kVjpFoldFloats = kHeads * 2 * kHidden * 4;      // d_fold: [heads][layer 0 / 2][512][4] (sdf_mlp_vjp_kernel.h)
static constexpr int kShortClusters = kClusterCap / kWavePts * kHeads;      // 128
static constexpr int kNearCap = ASDF_NEAR_CAP;      // near-level refinement list of a split-half sweep
static constexpr int kCandCap = ASDF_CAND_CAP;      // box candidates of asdf_decode_grid_box (a head without a certainly negative voxel - a thin
                                              // or tiny shape - lists its whole surface shell); shares near_idx
static constexpr int kAuditCap = 1 << 18;
static constexpr int kCandDirect = 1 << 15;  // candidates of a box-only sweep that go straight to the fp32 chain (more: split-half kernel first)
static constexpr int kBandCap = ASDF_BAND_CAP;     // voxels per head the narrow-band sweep re-evaluates at most (25 % of 256^3)

// SeparateDecoder: 2 MLPs x 1 output; CombinedDecoder: 1 MLP x 2 outputs
// (Re)build the one-plane image for the activation scales in force: constants block + the layer-1 / layer-2 records of the
// high-plane stream (see asdf_decoder::cst16p1).  Host work on ~1 M halves + two uploads; the caller has synchronised.
static hipError_t rebuild_one_plane(asdf_decoder* d) {
  if (!d->stream16_hi || !d->hi_host) return hipSuccess;
  const CstOffsets co = cst_offsets(d->kp);
  const size_t n = (size_t)kHeads * co.floats;
  std::memcpy(d->cst16p1_host, d->cst_host, n * sizeof(float));
  d->p1_usable = 1;
  std::memcpy(d->hi_scaled, d->hi_host, d->hi_count * sizeof(uint16_t));
  for (int h = 0; h < d->spec.num_heads; ++h) {
    const float sx0 = d->sx[h][0], sx1 = d->sx[h][1], sx2 = d->sx[h][2];
    // (the kernels' ReLU is c + |c| = 2 relu(c) - it keeps NaNs and infinities alive, sdf_mlp_f16_kernel.h - so the accumulators of
    // layers 0..2 carry HALF their activation's plane scale, and the last layer's weights the other 1 / 2 of its a w + |a| w form)
    const float sw1p = 0.5f * sx1 / sx0, sw2p = 0.5f * sx2 / sx1, sw3 = d->sw[h][2];
    const float* c = d->cst_host + (size_t)h * co.floats;
    float* o = d->cst16p1_host + (size_t)h * co.floats;
    for (int i = 0; i < kTilesL1 * 32; ++i) o[co.b1 + i] = c[co.b1 + i] * (sw1p * sx0);
    const float s3 = sw3 * sx2;
    for (int i = 0; i < kHidden; ++i) { o[co.b3 + i] = c[co.b3 + i] * s3; o[co.w4 + i] = 0.5f * c[co.w4 + i] / s3; o[co.w4b + i] = 0.5f * c[co.w4b + i] / s3; }
    o[co.b4] = c[co.b4]; o[co.b4 + 1] = c[co.b4 + 1];
    o[co.b4 + 2] = o[co.b4 + 3] = o[co.b4 + 4] = 1.0f;                       // (the multipliers of the split-half image: unused here)
    d->s0p[h] = 0.5f * sx0;
    d->s2p[h] = sw2p * sx1;
    if (d->spec.feature_mode == ASDF_FEATURES_NERF) {
      // the NeRF encoding's point-feature fragments are static weights (pack_decoder), not a per-sample fold: scaled here
      for (int i = 0; i < kTilesHidden * d->kp * 64; ++i) { o[co.a0 + i] = c[co.a0 + i] * d->s0p[h]; o[co.a2 + i] = c[co.a2 + i] * d->s2p[h]; }
    }
    // records of one head: [0, 256) layer 1, [256, 512) layer 2, [512, 1024) layer 3 (unchanged), 512 halves each
    const float f[2] = {sw1p / d->sw[h][0], sw2p / d->sw[h][1]};
    for (int l = 0; l < 2; ++l) {
      uint16_t* rec = d->hi_scaled + ((size_t)h * 1024 + (size_t)l * 256) * 512;
      float top = 0.0f;
      for (size_t i = 0; i < (size_t)256 * 512; ++i) {
        _Float16 v;
        std::memcpy(&v, rec + i, 2);
        const float w = (float)v * f[l];
        top = std::fmax(top, std::fabs(w));
        v = (_Float16)w;
        std::memcpy(rec + i, &v, 2);
      }
      // the largest weight must stay a comfortable fp16 number: below 2^15, and high enough that weights down to 2^-8 of it are
      // still normal (they carry the product sums; smaller ones go subnormal, 2^-25 absolute - far below the one-plane error)
      if (!(top < 32768.0f) || !(top >= 0.015625f)) d->p1_usable = 0;
    }
  }
  hipError_t e = hipMemcpy(d->cst16p1, d->cst16p1_host, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d->stream16_hi, d->hi_scaled, d->hi_count * sizeof(uint16_t), hipMemcpyHostToDevice);
  return e;
}

static bool spec_supported(const asdf_decoder_spec_t* s) {
  if (s->latent_size != kLatent || s->hidden != kHidden) return false;
  if (s->feature_mode == ASDF_FEATURES_NERF) {
    if (s->point_feats[0] != 9 && s->point_feats[0] != 15) return false;
    if (s->num_heads == 2 && s->point_feats[1] != s->point_feats[0]) return false;
  } else if (s->feature_mode != ASDF_FEATURES_AFFINE) {
    return false;
  }
  if (s->num_heads == 2) return s->outputs[0] == 1 && s->outputs[1] == 1;
  if (s->num_heads == 1) return s->outputs[0] == 2;
  return false;
}

static int set_sample_fold(asdf_decoder_t* d, const float* latent_dev, hipStream_t st) {
  FoldParams fp;
  fp.wlat = d->wlat; fp.wpt = d->wpt; fp.bias02 = d->bias02; fp.embed = d->embed; fp.latent = latent_dev;
  fp.kp = d->kp;
  int images = 1;
  fp.cst[0] = d->cst; fp.cst[1] = fp.cst[2] = nullptr;
  for (int h = 0; h < kHeads; ++h) {
    fp.pf[h] = h < d->spec.num_heads ? d->spec.point_feats[h] : 0;
    for (int i = 0; i < 3; ++i) { fp.s2[i][h] = 1.0f; fp.s0[i][h] = 1.0f; }
  }
  if (d->cst16) {      // the same fold into the split-half image, layer-2 constants scaled
    fp.cst[1] = d->cst16;
    for (int h = 0; h < kHeads; ++h) fp.s2[1][h] = d->s2[h];
    images = 2;
    if (d->cst16p1) {
      // ... and into the one-plane image (its own scales), whose layer-0 constants then become the kernels' fp16 point-feature /
      // bias operands (affine features; the NeRF-encoded kernels read them from the constants block as they are)
      fp.cst[2] = d->cst16p1;
      for (int h = 0; h < kHeads; ++h) { fp.s2[2][h] = d->s2p[h]; fp.s0[2][h] = d->s0p[h]; }
      images = 3;
    }
  }
  hipLaunchKernelGGL(fold_sample_kernel, dim3(d->spec.num_heads * 2 * kHidden / 4, images), dim3(256), 0, st, fp);
  if (images == 3 && d->a16) hipLaunchKernelGGL(fold_points_f16_kernel, dim3(d->spec.num_heads * 2), dim3(512), 0, st, d->cst16p1, d->a16, d->status);
  ASDF_HIP(hipGetLastError());
  d->sample_bound = true;
  return ASDF_OK;
}

// K1 in its subset mode over one voxel list: both MLPs of a SeparateDecoder concurrently (one launch each, the second on the
// decoder's side stream, joined back into `st`), everything else as one launch
static int launch_subset(asdf_decoder* d, const DecodeParams& q_in, bool two_out, int grid, hipStream_t st) {
  DecodeParams q = q_in;
  if (d->kp == 2 && d->short_max > 0 && q.mode == kGridSubset) {
    // short lists (the usual case of a near-level refinement: a few dozen to a few hundred voxels) take the short-list form - a
    // quarter of the tile form's latency; both are enqueued, the device-side count decides which one runs (bit-identical results)
    q.short_max = d->short_max;
    ShortParams sp = d->shortp;
    if (sp.cluster_max > d->short_max) sp.cluster_max = d->short_max;
    if (d->num_cus < 64) sp.cluster_max = 0;       // (its members wait for each other: they need workgroup slots side by side)
    // four workgroups per block and MLP, one per compute unit (155 KB of LDS each): beyond 64 blocks x MLPs the cluster form needs a
    // second round of the chip and loses to the short form's single one (N = 128 trace: 1 400 candidates x 2 MLPs, 0.22 -> 0.36 ms per
    // sample) - lists of up to 2048 / MLPs voxels take it
    if (sp.cluster_max > kClusterCap / q.num_mlps) sp.cluster_max = kClusterCap / q.num_mlps;
    if (!sp.fault) sp.cluster_max = 0;
    // a cluster launch that timed out waiting for a member writes nothing and raises *sp.fault: the tile form below - enqueued anyway,
    // it returns at once for a short list - then evaluates the list (same bits)
    q.short_fault = sp.cluster_max > 0 ? sp.fault : nullptr;
    k1_short_launch(two_out, q, sp, st);
  }
  if (two_out || q.num_mlps != 2 || !q.sdf0 || !q.sdf1 || !d->side) {
    k1_launch(d->kp, two_out, q, grid, st);
    return ASDF_OK;
  }
  DecodeParams q0 = q, q1 = q;
  q0.num_mlps = 1; q0.first_mlp = 0; q0.sdf1 = nullptr;
  q1.num_mlps = 1; q1.first_mlp = 1; q1.sdf0 = nullptr;
  ASDF_HIP(hipEventRecord(d->ev_fork, st));
  ASDF_HIP(hipStreamWaitEvent(d->side, d->ev_fork, 0));
  k1_launch(d->kp, false, q0, grid, st);
  k1_launch(d->kp, false, q1, grid, d->side);
  ASDF_HIP(hipEventRecord(d->ev_join, d->side));
  ASDF_HIP(hipStreamWaitEvent(st, d->ev_join, 0));
  return ASDF_OK;
}

// The voxel-list launch behind a sweep: the sweep's parameters `p` with another weights image (stream, cst) and the list, its count
// word and its capacity in place of the lattice; *grid = the workgroups of a launch over that capacity.
static DecodeParams list_params(const asdf_decoder* d, const DecodeParams& p, const float* stream, const float* cst, const int* idx,
                                const int* count_dev, int cap, int* grid) {
  DecodeParams q = p;
  q.stream = stream; q.cst = cst;
  q.mode = kGridSubset; q.grid_mode = p.mode; q.idx = idx; q.count_dev = count_dev; q.P = cap;
  *grid = cap / kWgPts < d->num_cus ? cap / kWgPts : d->num_cus;
  return q;
}

// `launch` (the dominant kernel of a sweep) between the one-shot event pair of asdf_decoder_time_next_sweep
template <class F>
static int timed_launch(asdf_decoder* d, hipStream_t st, F launch) {
  if (d->ev_start) ASDF_HIP(hipEventRecord((hipEvent_t)d->ev_start, st));
  launch();
  if (d->ev_stop) ASDF_HIP(hipEventRecord((hipEvent_t)d->ev_stop, st));
  d->ev_start = d->ev_stop = nullptr;
  return ASDF_OK;
}

static int launch_decode(asdf_decoder_t* d, DecodeParams& p, hipStream_t st) {
  if (!d->sample_bound) return ASDF_EINVAL;
  p.stream = d->stream;
  p.cst = d->cst;
  p.status = d->status;
  // a SeparateDecoder head whose output pointer is NULL is not evaluated at all (the reference always runs both,
  // networks/model.py:304-344, and discards one when HandBranch / ObjectBranch is off)
  p.first_mlp = 0;
  p.num_mlps = d->spec.num_heads;
  const bool two_out = d->spec.num_heads == 1;     // CombinedDecoder: one MLP, two last-layer rows
  if (p.bbox) {
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, p.bbox);
    ASDF_HIP(hipGetLastError());
  }
  const bool want_cls = p.logits || p.labels;
  // a pixel-aligned sample: the fp32 chain's PA form only (lattice sweeps and point lists; no label pass, no voxel lists)
  if (d->pixel_bound && (want_cls || d->math != ASDF_MATH_F32 || p.mode == kGridSubset || two_out)) return ASDF_EINVAL;
  if (!two_out) {
    if (!p.sdf0 && !p.sdf1 && !want_cls) return ASDF_OK;
    if (!p.sdf1) p.num_mlps = 1;
    else if (!p.sdf0) { p.first_mlp = 1; p.num_mlps = 1; }
  }
  const long long ntiles = (p.P + kWgPts - 1) / kWgPts;
  if (ntiles == 0) return ASDF_OK;
  const int grid = (int)(ntiles < d->num_cus ? ntiles : d->num_cus);
  p.pf = d->spec.point_feats[0];
  if (p.logits || p.labels) {
    // label pass: the classifier reads MLP 0's last hidden activation, so MLP 0 always runs
    if (!d->cls) return ASDF_EINVAL;
    p.cls = d->cls;
    p.num_class = d->num_class;
    if (!two_out && p.first_mlp != 0) { p.first_mlp = 0; p.num_mlps = 2; }
    k1_cls_launch(d->kp, two_out, p, grid, st);
    ASDF_HIP(hipGetLastError());
    return ASDF_OK;
  }
  // split-half arithmetic: grid sweeps only; the fp16 range report goes to the decoder's status word (asdf_decoder_status)
  // and, when the caller passed one, to word 7 / 15 of the bbox record it reads back anyway.  Explicit point lists (the
  // label pass, a few 10^4 points) stay on the fp32 chain
  if (d->math == ASDF_MATH_F16X3 && d->stream16 && p.mode != kPointList) {
    p.stream = d->stream16;
    p.cst = d->cst16;
    ASDF_TRY(timed_launch(d, st, [&] { k1h_launch(d->kp, two_out, p, grid, st); }));
    if (d->refine_tau > 0.0f && p.P <= 0x7fffffffLL) {
      // Near-level refinement: the split-half result and the exact fp32 FMA chain differ by a few 1e-7, so the SIGN of a
      // voxel within that distance of the iso level - all that marching cubes and the negative-voxel box look at - could
      // depend on the arithmetic.  Every voxel with |sdf| < tau (a few hundred of 16.7 M at N = 256) is re-evaluated on
      // the fp32 MFMA chain (the same kernel as ASDF_MATH_F32, coordinates from the same device function) and written
      // back in place: surfaces and boxes are those of the fp32 chain.
      ASDF_HIP(hipMemsetAsync(d->near_count, 0, sizeof(int), st));
      ASDF_HIP(hipMemsetAsync(d->status + ASDF_STATUS_LIST_OVERFLOW, 0, 2 * sizeof(int), st));  // this sweep's list-overflow count and "box may shrink" flag
      const long long n4 = (p.P + 3) / 4;
      const int cgrid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
      hipLaunchKernelGGL(collect_near_level_kernel, dim3(cgrid), dim3(256), 0, st, p.sdf0, p.sdf1, p.P, d->refine_tau, d->near_idx,
                         d->near_count, kNearCap, d->status);
      int rgrid;
      DecodeParams q = list_params(d, p, d->stream, d->cst, d->near_idx, d->near_count, kNearCap, &rgrid);
      q.fixup_flag = p.bbox ? d->status + ASDF_STATUS_FIXUP : nullptr;
      ASDF_TRY(launch_subset(d, q, two_out, rgrid, st));
      if (p.bbox) {
        // the fused box saw the unrefined values.  The refinement pass patches it in place - a voxel that became negative
        // extends the box and the count exactly - and raises a flag when one became non-negative (the box may have to
        // shrink): only then do the three kernels below recount on the refined volumes (the range report words stay).
        const int* flag = d->status + ASDF_STATUS_FIXUP;
        hipLaunchKernelGGL(bbox_reinit_keep_flags_kernel, dim3(1), dim3(64), 0, st, p.bbox, flag);
        const long long rows = (long long)p.N * p.N;
        const int bgrid = (int)((rows + 3) / 4 < 1024 ? (rows + 3) / 4 : 1024);
        if (p.sdf0) hipLaunchKernelGGL(neg_bbox_kernel, dim3(bgrid), dim3(256), 0, st, p.sdf0, p.N, p.N, p.N, p.bbox, flag);
        if (p.sdf1) hipLaunchKernelGGL(neg_bbox_kernel, dim3(bgrid), dim3(256), 0, st, p.sdf1, p.N, p.N, p.N, p.bbox + ASDF_BOX_STRIDE, flag);
        hipLaunchKernelGGL(near_overflow_to_bbox_kernel, dim3(1), dim3(64), 0, st, d->status, p.bbox);
      }
    }
  } else {
    ASDF_TRY(timed_launch(d, st, [&] {
      if (d->pixel_bound) k1pa_launch(p, d->pixel, grid, st);
      else k1_launch(d->kp, two_out, p, grid, st);
    }));
  }
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

// (origin / voxel_size by value, or - lattice_dev non-null - {origin0, origin1, origin2, voxel} read by the kernels from device memory)
static int decode_grid_impl(asdf_decoder_t* d, int32_t N, const float* origin, float voxel_size, const float* lattice_dev, int32_t grid_mode,
                            float* sdf_hand_dev, float* sdf_obj_dev, int32_t* bbox_dev, void* stream) {
  if (!d || (!origin && !lattice_dev) || N < 2 || N > 1024) return ASDF_EINVAL;
  if (grid_mode != ASDF_GRID_REFERENCE && grid_mode != ASDF_GRID_INTEGER) return ASDF_EINVAL;
  DecodeParams p;
  std::memset(&p, 0, sizeof(p));
  p.sdf0 = sdf_hand_dev; p.sdf1 = sdf_obj_dev; p.bbox = bbox_dev;
  p.P = (long long)N * N * N; p.N = N; p.mode = grid_mode == ASDF_GRID_REFERENCE ? kGridReference : kGridInteger;
  if (lattice_dev) p.lattice = lattice_dev;
  else { p.vs = voxel_size; p.o0 = origin[0]; p.o1 = origin[1]; p.o2 = origin[2]; }
  return launch_decode(d, p, (hipStream_t)stream);
}

// the audit of a one-plane sweep: min(d->audit_n, P / 64) voxels the sweep decided by sign alone are appended to list[*count ..] -
// half of them drawn uniformly (audit_pick_kernel), half from the at-risk shell (shell_count_kernel / shell_pick_kernel) - and the
// seed advances.  The small lattices pay a share of their own size, not a sample sized for 256^3 (round 5: a
// 64th - still four times the share of the lattice that 65 536 picks are at N = 256.  At a sixteenth a 128^3 lattice paid the full
// 256^3 sample, 5 % of its sample time.  The shell half stays exhaustive wherever the shell is smaller than its budget - hundreds to
// thousands of voxels on these lattices - and the uniform half's size enters the tail ratio the estimate is corrected with).
static int audit_size(const asdf_decoder* d, long long P) {
  if (d->audit_n <= 0) return 0;
  const long long cap = P / 64 > 64 ? P / 64 : 64;
  return (long long)d->audit_n < cap ? d->audit_n : (int)cap;
}

static int enqueue_audit_picks(asdf_decoder* d, const float* a, const float* b, const unsigned char* mark, long long P, float tau,
                               int* list, int* count, int cap, int use, hipStream_t st) {
  const int n = audit_size(d, P);
  if (n <= 0) return ASDF_OK;
  const int uniform = n - n / 2, budget = n / 2;
  if (budget > 0) {
    // (the shell population of this use - head `use` of a band sweep, 0 for a box sweep: cleared with the record by sweep_init_kernel)
    int* shell_n = d->audit_rec + kAuditShellCount + use;
    const int sgrid = (int)((P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048);
    hipLaunchKernelGGL(shell_count_kernel, dim3(sgrid + (uniform + 255) / 256), dim3(256), 0, st, a, b, mark, P, tau, shell_n, sgrid,
                       d->audit_seed, uniform, list, count, cap);
    hipLaunchKernelGGL(shell_pick_kernel, dim3(sgrid), dim3(256), 0, st, a, b, mark, P, tau, d->audit_seed ^ 0xA5A5A5A55A5A5A5Aull, budget,
                       shell_n, list, count, cap, d->audit_rec);
  } else {
    hipLaunchKernelGGL(audit_pick_kernel, dim3((uniform + 255) / 256), dim3(256), 0, st, a, b, mark, P, tau, d->audit_seed, uniform,
                       list, count, cap);
  }
  ASDF_HIP(hipGetLastError());
  d->audit_seed = d->audit_seed * 6364136223846793005ull + 1442695040888963407ull;
  return ASDF_OK;
}

// What the box-only and the narrow-band sweep share: the checks of their arguments and the parameters of the one-plane sweep
// kernel over the lattice (origin / voxel_size by value, or - lattice_dev non-null - read by the kernels from device memory).
static int one_plane_params(const asdf_decoder* d, int32_t N, const float* origin, float voxel_size, const float* lattice_dev, int32_t grid_mode,
                            float tau, float* sdf_hand_dev, float* sdf_obj_dev, int32_t* rec_dev, DecodeParams& p) {
  if (!d || (!origin && !lattice_dev) || !rec_dev || N < 2 || N > 1024 || !(tau > 0.0f) || !(tau < 0.5f)) return ASDF_EINVAL;
  if (grid_mode != ASDF_GRID_REFERENCE && grid_mode != ASDF_GRID_INTEGER) return ASDF_EINVAL;
  if (!d->stream16_hi || !d->sample_bound || !d->p1_usable || d->pixel_bound) return ASDF_EINVAL;
  const bool two_out = d->spec.num_heads == 1;       // CombinedDecoder: one MLP, both columns from every evaluation
  if (two_out ? !(sdf_hand_dev && sdf_obj_dev) : (!sdf_hand_dev && !sdf_obj_dev)) return ASDF_EINVAL;
  std::memset(&p, 0, sizeof(p));
  p.sdf0 = sdf_hand_dev; p.sdf1 = sdf_obj_dev; p.bbox = rec_dev;      // (band sweep: the box words are by-products; the range words carry the range report)
  p.P = (long long)N * N * N; p.N = N; p.mode = grid_mode == ASDF_GRID_REFERENCE ? kGridReference : kGridInteger;
  if (lattice_dev) p.lattice = lattice_dev;        // (every list launch copies p: the listed voxels get the same lattice)
  else { p.vs = voxel_size; p.o0 = origin[0]; p.o1 = origin[1]; p.o2 = origin[2]; }
  p.stream = d->stream16_hi; p.cst = d->cst16p1; p.a16 = d->a16; p.status = d->status;
  p.first_mlp = 0; p.num_mlps = d->spec.num_heads; p.pf = d->spec.point_feats[0];
  if (!two_out) {
    if (!p.sdf1) p.num_mlps = 1;
    else if (!p.sdf0) { p.first_mlp = 1; p.num_mlps = 1; }
  }
  return ASDF_OK;
}

// ... and the sweep itself: the box record and the counter / flag words in `clear` start empty (the status words from
// ASDF_STATUS_LIST_OVERFLOW to ASDF_STATUS_MAX_ERR and the audit record always do; none of them is touched by the sweep kernel
// itself), then the one-plane kernel over the lattice
static int one_plane_sweep(asdf_decoder* d, const DecodeParams& p, ClearRange clear_a, ClearRange clear_b, hipStream_t st) {
  const bool two_out = d->spec.num_heads == 1;
  hipLaunchKernelGGL(sweep_init_kernel, dim3(1), dim3(64), 0, st, p.bbox, clear_a, ClearRange{d->status + ASDF_STATUS_LIST_OVERFLOW, 3},
                     ClearRange{d->audit_rec, kAuditWords}, clear_b);
  const long long ntiles = (p.P + kWgPts - 1) / kWgPts;
  const int grid = (int)(ntiles < d->num_cus ? ntiles : d->num_cus);
  return timed_launch(d, st, [&] {
    if (d->kp == 2) k1h_box_launch(two_out, p, grid, st);
    else k1s_nerf_launch(d->kp, two_out, p, grid, st);
  });
}

static int decode_grid_band_impl(asdf_decoder_t* d, int32_t N, const float* origin, float voxel_size, const float* lattice_dev,
                                 int32_t grid_mode, float tau, float* sdf_hand_dev, float* sdf_obj_dev, int32_t* rec_dev, void* stream) {
  DecodeParams p;
  ASDF_TRY(one_plane_params(d, N, origin, voxel_size, lattice_dev, grid_mode, tau, sdf_hand_dev, sdf_obj_dev, rec_dev, p));
  const bool two_out = d->spec.num_heads == 1;
  hipStream_t st = (hipStream_t)stream;
  const long long P = p.P;
  if (!d->band_idx) {
    ASDF_HIP(hipMalloc((void**)&d->band_idx, 2 * (size_t)kBandCap * sizeof(int)));
    ASDF_HIP(hipMalloc((void**)&d->band_count, 2 * sizeof(int)));
  }
  if (d->band_mark_bytes < (size_t)P + 16) {
    if (d->band_mark) ASDF_HIP(hipFree(d->band_mark));
    d->band_mark = nullptr; d->band_mark_bytes = 0;
    ASDF_HIP(hipMalloc((void**)&d->band_mark, (size_t)P + 16));
    d->band_mark_bytes = (size_t)P + 16;
  }
  // (cleared with the record: the two band counts and the near-level count)
  ASDF_TRY(one_plane_sweep(d, p, ClearRange{d->band_count, 2}, ClearRange{d->near_count, 1}, st));
  float* vols[2] = {sdf_hand_dev, sdf_obj_dev};
  // SeparateDecoder: one list per head (an MLP is evaluated for ITS marked voxels only).  CombinedDecoder (networks/model.py:149-188):
  // every evaluation yields both columns, so the corners of the cells that can be active in EITHER volume are marked into one list
  // (h = 0) and re-evaluated once.
  for (int h = 0; h < (two_out ? 1 : 2); ++h) {
    if (!vols[h]) continue;
    ASDF_HIP(hipMemsetAsync(d->band_mark, 0, (size_t)P, st));
    const int per_slab = (((N - 1) + 3) >> 2) * (N - 1);          // (y, group of four x-consecutive cells) pairs per z
    const dim3 mgrid((per_slab + 255) / 256, N - 1 < 1024 ? N - 1 : 1024);
    hipLaunchKernelGGL(band_mark_kernel, mgrid, dim3(256), 0, st, vols[h], N, tau, d->band_mark);
    if (two_out) hipLaunchKernelGGL(band_mark_kernel, mgrid, dim3(256), 0, st, vols[1], N, tau, d->band_mark);
    const long long items = (P + 15) / 16;
    const int cgrid = (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
    int* list = d->band_idx + (size_t)h * kBandCap;
    // the audit picks of this head - unmarked voxels, i.e. voxels marching cubes will read the SIGN of and nothing else - ride
    // behind the marked ones in the same list (positions >= audit word kAuditFrom + h: the compaction's last workgroup writes that word)
    // (... on the small lattices, where a launch is what counts.  On a large one the 4096 arrivals on one word cost more than the
    // 4-byte copy they replace - 19 -> 51 us per launch at N = 256 in the kernel statistics - so there the copy stays)
    const bool publish = cgrid <= 256;
    int* audit_from = d->audit_rec + kAuditFrom + h;
    hipLaunchKernelGGL(band_compact_kernel, dim3(cgrid), dim3(256), 0, st, d->band_mark, P, list, d->band_count + h, kBandCap,
                       publish ? d->audit_rec + kAuditCompactDone + h : nullptr, audit_from);
    if (!publish) ASDF_HIP(hipMemcpyAsync(audit_from, d->band_count + h, sizeof(int), hipMemcpyDeviceToDevice, st));
    ASDF_TRY(enqueue_audit_picks(d, vols[h], two_out ? vols[1] : nullptr, d->band_mark, P, tau, list, d->band_count + h, kBandCap, h, st));
    // the values of the ordinary sweep at the listed voxels of this head: the split-half kernel over the list ...
    int rgrid;
    DecodeParams q = list_params(d, p, d->stream16, d->cst16, list, d->band_count + h, kBandCap, &rgrid);
    q.bbox = nullptr; q.neg_thr = 0.0f;
    if (!two_out) { q.sdf0 = h == 0 ? vols[0] : nullptr; q.sdf1 = h == 1 ? vols[1] : nullptr; }
    q.first_mlp = two_out ? 0 : h; q.num_mlps = 1;
    q.audit = d->audit_n > 0 ? d->audit_rec : nullptr; q.audit_from = audit_from;
    k1h_subset_launch(d->kp, two_out, q, rgrid, st);
  }
  if (d->refine_tau > 0.0f) {
    // ... and, as behind every split-half sweep, the fp32 chain where those values lie within refine_tau of the level (both
    // MLPs over the union of the two near-level lists: an extra exact value is harmless)
    for (int h = 0; h < 2; ++h)
      if (vols[h]) {
        const int l = two_out ? 0 : h;       // (a CombinedDecoder's one list serves both volumes)
        hipLaunchKernelGGL(collect_near_level_list_kernel, dim3(256), dim3(256), 0, st, vols[h], d->band_idx + (size_t)l * kBandCap,
                           d->band_count + l, kBandCap, d->refine_tau, d->near_idx, d->near_count, kNearCap, d->status);
      }
    int ngrid;
    DecodeParams q = list_params(d, p, d->stream, d->cst, d->near_idx, d->near_count, kNearCap, &ngrid);
    q.bbox = nullptr; q.neg_thr = 0.0f; q.status = nullptr;
    ASDF_TRY(launch_subset(d, q, two_out, ngrid, st));
  }
  hipLaunchKernelGGL(sweep_record_kernel, dim3(1), dim3(64), 0, st, rec_dev, d->status, d->near_count, d->audit_rec);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

// What the point-list forms of the fp32 chain (gradient, reverse mode, fit, tracing, projection) cover: SeparateDecoder with affine point
// features and an ordinary (per-sample constant) latent.  (The reverse-mode forms also need the transposed weight image, d->streamT.)
static bool point_list_covered(const asdf_decoder* d) {
  return d->spec.num_heads == 2 && d->spec.feature_mode == ASDF_FEATURES_AFFINE && d->kp == 2 && !d->pixel_bound;
}

// ... and their launch over M points at xyz (null: the kernel has its own positions) for the heads of heads_mask (bit h: head h), with the
// constants block `cst`: always the fp32 chain's weights - d->math and the MFMA shape of the split-half sweeps are not looked at
static DecodeParams point_list_params(const asdf_decoder* d, const float* cst, const float* xyz, int64_t M, int heads_mask) {
  DecodeParams p;
  std::memset(&p, 0, sizeof(p));
  p.stream = d->stream; p.cst = cst;
  p.xyz = xyz; p.P = M; p.N = 1; p.mode = kPointList;
  p.first_mlp = (heads_mask & 1) ? 0 : 1;
  p.num_mlps = heads_mask == 3 ? 2 : 1;
  p.pf = d->spec.point_feats[0];
  return p;
}

// ---- the fit (k1_launch.h: THE FIT): one loop for asdf_fit_codes and its batch of one, asdf_fit_code --------------------------------------
// sample `first .. first + m` of the concatenated lists, whose workgroups start at wg0 of the launch; nh / no = the sizes of its heads'
// sets.  A head with an empty set is absent; a sample without heads has no workgroups (only the prior moves its code).
static FitSampleDesc fit_describe(const asdf_decoder* d, int first, int64_t m, int wg0, int64_t nh, int64_t no) {
  FitSampleDesc sd;
  std::memset(&sd, 0, sizeof(sd));
  sd.first = first; sd.m = (int)m; sd.wg0 = wg0;
  sd.heads_mask = (nh > 0 ? 1 : 0) | (no > 0 ? 2 : 0);
  sd.grid = sd.heads_mask ? k1v_grid(m, d->num_cus) : 0;
  sd.inv_n_d[0] = nh > 0 ? 1.0 / (double)nh : 0.0; sd.inv_n_d[1] = no > 0 ? 1.0 / (double)no : 0.0;
  sd.inv_n[0] = (float)sd.inv_n_d[0]; sd.inv_n[1] = (float)sd.inv_n_d[1];
  return sd;
}

struct FitBuffers {          // device memory of a fit over B samples
  FitSampleDesc* samples;    // [B] and
  FitWg* wgs;                // [sum of grids]: written here from the host's descriptors
  const float* cst;          // [B][heads][kCstFloats] the constants blocks `fold` writes
  float* partial;            // [sum of grids][kVjpFoldFloats]
  float* fold;               // [B][kVjpFoldFloats] d_fold
  double* loss_partial;      // [sum of grids][heads]
  float* state;              // [B][kFitStateFloats] the Adam states
  const float* xyz;          // the samples' lists one behind the other, and
  const float* t[2];         // their targets per head (null: no sample has that head)
  float* z;                  // [B][kLatent] in: the start codes, out: the fitted ones
  const float* z0;           // [B][kLatent] (null: the start codes)
  const float* step_table;   // [steps][2]
  double* history;           // [B][steps] (null: not wanted)
};

// `steps` steps on the B samples of descs; fold() -> ASDF_* brings the constants blocks up to z before each step's loss launch
template <class F>
static int fit_loop(asdf_decoder* d, const FitSampleDesc* descs, int B, const FitBuffers& b, float clamp, float prior, int steps, hipStream_t st,
                    F fold) {
  const int total_wgs = descs[B - 1].wg0 + descs[B - 1].grid;
  // (each workgroup of the loss form takes P, first_mlp, num_mlps and inv_n from its sample's descriptor)
  const DecodeParams p = point_list_params(d, b.cst, b.xyz, 0, 3);
  VjpParams v;
  v.streamT = d->streamT; v.w[0] = b.t[0]; v.w[1] = b.t[1]; v.partial = b.partial;
  VjpLossParams q;
  q.clamp = clamp; q.inv_n[0] = q.inv_n[1] = 0.0f; q.partial = b.loss_partial;
  VjpBatchParams vb;
  vb.samples = b.samples; vb.wgs = b.wgs; vb.cst = b.cst;
  AdamRule rule;
  rule.b1 = 0.9f; rule.b2 = 0.999f; rule.eps = 1e-8f; rule.k_prior = (float)(2.0 * (double)prior / kLatent);
  k1vb_describe(descs, B, b.samples, b.wgs, st);
  k1vb_adam_init(b.state, b.z, b.z0, B, st);
  for (int k = 0; k < steps; ++k) {
    ASDF_TRY(fold());
    if (total_wgs > 0) k1vb_loss_launch(p, v, q, vb, total_wgs, st);
    k1vb_finish_loss(b.samples, B, b.partial, b.loss_partial, b.fold, d->wlat, d->wpt, ASDF_MAX_POINT_FEATS, b.state,
                     b.history ? b.history + k : nullptr, steps, st);
    k1vb_adam_step(b.state, b.step_table + 2 * (size_t)k, rule, b.z, B, st);
  }
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

extern "C" {

int asdf_version(void) { return 132; }      // (asdf_project_points is an addition: no existing call changed)

int asdf_set_mfma_shape(int shape) {
  if (shape != 0 && shape != 16 && shape != 32) return ASDF_EINVAL;
  return k1h_set_shape(shape);
}
int asdf_get_mfma_shape(void) { return k1h_shape(); }

const char* asdf_strerror(int code) {
  switch (code) {
    case ASDF_OK: return "ok";
    case ASDF_EINVAL: return "invalid argument or unsupported decoder shape";
    case ASDF_ENOMEM: return "out of memory";
    case ASDF_EHIP: return "HIP runtime error";
    case ASDF_ENODEV: return "no gfx950 device";
    case ASDF_ENOSPC: return "buffer or workspace too small";
    case ASDF_ERANGE: return "Surface level must be within volume data range.";
    case ASDF_ENOSURF: return "No surface found at the given iso value.";
    case ASDF_ENOGRAD: return "the gradient kernel does not cover this decoder (SeparateDecoder with affine point features only)";
    case ASDF_ENOTRACE: return "the ray-tracing kernel does not cover this decoder (SeparateDecoder with affine point features only)";
    case ASDF_ENOPROJECT: return "the projection kernel does not cover this decoder (SeparateDecoder with affine point features only)";
    default: return "unknown error";
  }
}

int asdf_last_hip_error(void) { return g_last_hip_error; }

int asdf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int good = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

void asdf_decoder_destroy(asdf_decoder_t* d) {
  if (!d) return;
  for (hipStream_t side : {d->side, d->audit_side})
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
  for (hipEvent_t ev : {d->ev_audit_fork, d->ev_audit_join, d->ev_fork, d->ev_join})
    if (ev) (void)hipEventDestroy(ev);
  void* bufs[] = {d->stream, d->wlat, d->wpt, d->bias02, d->cst, d->embed, d->cls, d->stream16, d->cst16, d->stream16_hi, d->a16, d->cst16p1,
                  d->pa_proj, d->pa_cstb, d->pa_ws, d->pa_lat, d->shortp.xchg, d->shortp.arrivals, d->band_mark, d->box_aux, d->band_idx,
                  d->band_count, d->status, d->latent_stage, d->near_idx, d->near_count, d->audit_rec, d->audit_idx, d->audit_count,
                  d->trace_queue, d->streamT, d->vjp_partial};
  for (void* b : bufs) (void)hipFree(b);       // (a null pointer is a no-op)
  std::free(d->cst_host);
  std::free(d->cst16_host);
  std::free(d->cst16p1_host);
  std::free(d->hi_host);
  std::free(d->hi_scaled);
  delete d;
}

int asdf_decoder_create(const asdf_decoder_spec_t* spec, const asdf_head_params_t* heads, asdf_decoder_t** out) {
  if (!spec || !heads || !out) return ASDF_EINVAL;
  *out = nullptr;
  if (!spec_supported(spec)) return ASDF_EINVAL;
  for (int h = 0; h < spec->num_heads; ++h) {
    if (spec->point_feats[h] < 1 || spec->point_feats[h] > ASDF_MAX_POINT_FEATS) return ASDF_EINVAL;
    if (kHidden - kLatent - spec->point_feats[h] < 1) return ASDF_EINVAL;
    for (int l = 0; l < 5; ++l)
      if (!heads[h].w[l] || !heads[h].b[l]) return ASDF_EINVAL;
  }
  int dev = 0;
  ASDF_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  ASDF_HIP(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ASDF_ENODEV;

  asdf_decoder* d = new (std::nothrow) asdf_decoder();
  if (!d) return ASDF_ENOMEM;
  std::memset(d, 0, sizeof(*d));
  d->spec = *spec;
  d->device = dev;
  d->num_cus = prop.multiProcessorCount;

  HostPack hp;
  if (!pack_decoder(*spec, heads, hp)) { delete d; return ASDF_ENOMEM; }
  d->kp = hp.kp;
  std::vector<float>&stream = hp.stream, &wlat = hp.wlat, &wpt = hp.wpt, &b02 = hp.b02, &cst = hp.cst, &emb = hp.emb;

  hipError_t e = hipSuccess;
  auto up = [&](float** dst, const std::vector<float>& src) {
    if (e != hipSuccess) return;
    e = hipMalloc((void**)dst, src.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice);
  };
  up(&d->stream, stream); up(&d->wlat, wlat); up(&d->wpt, wpt); up(&d->bias02, b02); up(&d->cst, cst); up(&d->embed, emb);
  if (!hp.streamT.empty() && d->kp == 2) up(&d->streamT, hp.streamT);
  d->math = ASDF_MATH_F32;
  if (e == hipSuccess) {
    if (!pack_decoder_f16(*spec, heads, hp)) { asdf_decoder_destroy(d); return ASDF_ENOMEM; }
    up(&d->cst16, hp.cst16);
    // (one allocation: the 32x32x16 image, and behind it the W form's - its kernels add the offset themselves)
    if (e == hipSuccess) e = hipMalloc((void**)&d->stream16, (hp.stream16.size() + hp.stream16w.size()) * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d->stream16, hp.stream16.data(), hp.stream16.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(reinterpret_cast<uint16_t*>(d->stream16) + hp.stream16.size(), hp.stream16w.data(),
                                       hp.stream16w.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      // records of [plane hi / lo][lane][8 halves] -> the hi halves alone, same record order
      const size_t nrec = hp.stream16.size() / 1024;
      std::vector<uint16_t> hi(nrec * 512);
      for (size_t r = 0; r < nrec; ++r) std::memcpy(&hi[r * 512], &hp.stream16[r * 1024], 512 * sizeof(uint16_t));
      e = hipMalloc((void**)&d->stream16_hi, hi.size() * sizeof(uint16_t));
      if (e == hipSuccess) e = hipMemcpy(d->stream16_hi, hi.data(), hi.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
      d->hi_count = hi.size();
      d->hi_host = (uint16_t*)std::malloc(hi.size() * sizeof(uint16_t));
      d->hi_scaled = (uint16_t*)std::malloc(hi.size() * sizeof(uint16_t));
      d->cst16p1_host = (float*)std::malloc(hp.cst.size() * sizeof(float));
      if (!d->hi_host || !d->hi_scaled || !d->cst16p1_host) { asdf_decoder_destroy(d); return ASDF_ENOMEM; }
      std::memcpy(d->hi_host, hi.data(), hi.size() * sizeof(uint16_t));
      if (e == hipSuccess) e = hipMalloc((void**)&d->cst16p1, hp.cst.size() * sizeof(float));
      if (e == hipSuccess && d->kp == 2) {      // (affine point features: layer 0's bias row and point columns as one fp16 A operand, K0b)
        e = hipMalloc((void**)&d->a16, (size_t)kHeads * kA16Floats * sizeof(float));
        if (e == hipSuccess) e = hipMemset(d->a16, 0, (size_t)kHeads * kA16Floats * sizeof(float));
      }
    }
    for (int h = 0; h < kHeads; ++h) {
      d->s2[h] = h < spec->num_heads ? hp.s2[h] : 1.0f;
      for (int l = 0; l < 3; ++l) { d->sw[h][l] = h < spec->num_heads ? hp.sw[h][l] : 1.0f; d->sx[h][l] = kActScale; }
    }
    d->cst_host = (float*)std::malloc(hp.cst.size() * sizeof(float));
    d->cst16_host = (float*)std::malloc(hp.cst.size() * sizeof(float));
    if (!d->cst_host || !d->cst16_host) { asdf_decoder_destroy(d); return ASDF_ENOMEM; }
    std::memcpy(d->cst_host, hp.cst.data(), hp.cst.size() * sizeof(float));
    if (e == hipSuccess) e = rebuild_one_plane(d);          // the one-plane image at the default activation scales
    if (e == hipSuccess) e = k1h_prepare();
    if (e == hipSuccess) e = k1s_nerf_prepare();
  }
  if (e == hipSuccess) e = k1_prepare();
  if (e == hipSuccess) e = k1_cls_prepare();
  if (e == hipSuccess) e = k1pa_prepare();
  if (e == hipSuccess) e = k1g_prepare();
  if (e == hipSuccess) e = k1t_prepare();
  if (e == hipSuccess) e = k1p_prepare();
  if (e == hipSuccess) e = k1v_prepare();
  if (e == hipSuccess) e = k1vb_prepare();
  if (e == hipSuccess) e = hipMalloc((void**)&d->trace_queue, 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&d->latent_stage, kLatent * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d->status, ASDF_STATUS_WORDS * sizeof(int));
  if (e == hipSuccess) e = hipMemset(d->status, 0, ASDF_STATUS_WORDS * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d->near_idx, kCandCap * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d->near_count, sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d->audit_rec, kAuditWords * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d->audit_idx, kAuditCap * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d->audit_count, sizeof(int));
  d->audit_n = 1 << 16;
  d->audit_seed = 0x5DF5A11D00000000ull;
  d->short_max = 8192;
  d->shortp.cluster_max = kClusterCap;
  d->shortp.fault = d->status ? d->status + ASDF_STATUS_CLUSTER_FAULT : nullptr;
  d->shortp.timeout_ticks = kClusterTimeoutTicks;
  if (e == hipSuccess) e = hipMalloc((void**)&d->shortp.xchg, (size_t)kShortClusters * kXchgFloats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d->shortp.arrivals, (size_t)kShortClusters * 4 * sizeof(int));
  if (e == hipSuccess) e = hipMemset(d->shortp.arrivals, 0, (size_t)kShortClusters * 4 * sizeof(int));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->audit_side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_audit_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_audit_join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming);
  d->refine_tau = 4e-6f;

  if (e != hipSuccess) {
    g_last_hip_error = (int)e;
    asdf_decoder_destroy(d);
    return e == hipErrorOutOfMemory ? ASDF_ENOMEM : ASDF_EHIP;
  }
  *out = d;
  return ASDF_OK;
}

int asdf_neg_bbox(const float* vol_dev, int32_t n0, int32_t n1, int32_t n2, int32_t* bbox_dev, void* stream) {
  if (!vol_dev || !bbox_dev || n0 < 1 || n1 < 1 || n2 < 1) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, bbox_dev);
  const long long rows = (long long)n0 * n1;
  const int grid = (int)((rows + 3) / 4 < 1024 ? (rows + 3) / 4 : 1024);
  hipLaunchKernelGGL(neg_bbox_kernel, dim3(grid), dim3(256), 0, st, vol_dev, n0, n1, n2, bbox_dev, (const int*)nullptr);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_debug_pack_host(const asdf_decoder_spec_t* spec, const asdf_head_params_t* heads, float* stream,
                         float* wlat, float* wpt, float* bias02, float* cst, float* embed) {
  if (!spec || !heads || !spec_supported(spec)) return ASDF_EINVAL;
  HostPack hp;
  if (!pack_decoder(*spec, heads, hp)) return ASDF_ENOMEM;
  auto cp = [](float* dst, const std::vector<float>& v) { if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(float)); };
  cp(stream, hp.stream); cp(wlat, hp.wlat); cp(wpt, hp.wpt); cp(bias02, hp.b02); cp(cst, hp.cst); cp(embed, hp.emb);
  return ASDF_OK;
}

int asdf_debug_pack_host_f16w(const asdf_decoder_spec_t* spec, const asdf_head_params_t* heads, uint16_t* stream16w) {
  if (!spec || !heads || !stream16w || !spec_supported(spec)) return ASDF_EINVAL;
  HostPack hp;
  if (!pack_decoder(*spec, heads, hp)) return ASDF_ENOMEM;
  if (!pack_decoder_f16(*spec, heads, hp)) return ASDF_ENOMEM;
  std::memcpy(stream16w, hp.stream16w.data(), hp.stream16w.size() * sizeof(uint16_t));
  return ASDF_OK;
}

int asdf_debug_pack_host_f16(const asdf_decoder_spec_t* spec, const asdf_head_params_t* heads, uint16_t* stream16, float* cst16,
                             float* s2) {
  if (!spec || !heads || !spec_supported(spec)) return ASDF_EINVAL;
  HostPack hp;
  if (!pack_decoder(*spec, heads, hp)) return ASDF_ENOMEM;
  if (!pack_decoder_f16(*spec, heads, hp)) return ASDF_ENOMEM;
  if (stream16) std::memcpy(stream16, hp.stream16.data(), hp.stream16.size() * sizeof(uint16_t));
  if (cst16) std::memcpy(cst16, hp.cst16.data(), hp.cst16.size() * sizeof(float));
  if (s2) for (int h = 0; h < kHeads; ++h) s2[h] = h < spec->num_heads ? hp.s2[h] : 1.0f;
  return ASDF_OK;
}

int asdf_decoder_set_sample(asdf_decoder_t* d, const float* latent_dev, const float* embed_host, void* stream) {
  if (!d || !latent_dev) return ASDF_EINVAL;
  if (embed_host && d->spec.feature_mode != ASDF_FEATURES_AFFINE) return ASDF_EINVAL;
  d->pixel_bound = false;
  hipStream_t st = (hipStream_t)stream;
  if (embed_host) {
    ASDF_HIP(hipMemcpyAsync(d->embed, embed_host, sizeof(float) * kHeads * ASDF_MAX_POINT_FEATS * 4,
                            hipMemcpyHostToDevice, st));
  }
  return set_sample_fold(d, latent_dev, st);
}

int asdf_decoder_set_sample_host(asdf_decoder_t* d, const float* latent_pinned, const float* embed_pinned, void* stream) {
  if (!d || !latent_pinned || !d->latent_stage) return ASDF_EINVAL;
  if (embed_pinned && d->spec.feature_mode != ASDF_FEATURES_AFFINE) return ASDF_EINVAL;
  d->pixel_bound = false;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stage_sample_kernel, dim3(1), dim3(256), 0, st, latent_pinned, embed_pinned, d->latent_stage, d->embed,
                     kHeads * ASDF_MAX_POINT_FEATS * 4);
  ASDF_HIP(hipGetLastError());
  return set_sample_fold(d, d->latent_stage, st);
}

int asdf_decoder_set_sample_pixel(asdf_decoder_t* d, const float* feat_dev, int32_t C, int32_t H, int32_t W, const float cam3x4[12],
                                  const float root3[3], float image_size, float scale_factor, void* stream) {
  if (!d || !feat_dev || !cam3x4 || !root3) return ASDF_EINVAL;
  if (C != d->spec.latent_size || H < 1 || H > 256 || W < 1 || W > 256) return ASDF_EINVAL;
  if (!(image_size > 0.0f) || !(scale_factor > 0.0f)) return ASDF_EINVAL;
  // SeparateDecoder with xyz point features only (the PA form of the fp32 chain: k1pa_kernels.hip)
  if (d->spec.num_heads != 2 || d->spec.feature_mode != ASDF_FEATURES_AFFINE || d->kp != 2 || d->spec.point_feats[0] != 3 ||
      d->spec.point_feats[1] != 3)
    return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (d->streamT) {
    // a decoder that binds pixel-aligned samples is one the reverse-mode form never accepts: its transposed weight image (4 MiB) goes
    ASDF_HIP(hipDeviceSynchronize());
    ASDF_HIP(hipFree(d->streamT));
    d->streamT = nullptr;
  }
  const CstOffsets co = cst_offsets(2);
  const size_t hw = (size_t)H * W, need = (size_t)kHeads * 2 * hw * kHidden;
  if (need > d->pa_proj_floats) {
    if (d->pa_proj) { ASDF_HIP(hipStreamSynchronize(st)); ASDF_HIP(hipFree(d->pa_proj)); d->pa_proj = nullptr; d->pa_proj_floats = 0; }
    ASDF_HIP(hipMalloc((void**)&d->pa_proj, need * sizeof(float)));
    d->pa_proj_floats = need;
  }
  if (!d->pa_cstb) {
    ASDF_HIP(hipMalloc((void**)&d->pa_cstb, (size_t)kHeads * co.floats * sizeof(float)));
    ASDF_HIP(hipMemcpy(d->pa_cstb, d->cst, (size_t)kHeads * co.floats * sizeof(float), hipMemcpyDeviceToDevice));
    ASDF_HIP(hipMalloc((void**)&d->pa_ws, (size_t)d->num_cus * kPixelWsFloats * sizeof(float)));
    ASDF_HIP(hipMalloc((void**)&d->pa_lat, 2 * kLatent * sizeof(float)));
    ASDF_HIP(hipMemset(d->pa_lat, 0, 2 * kLatent * sizeof(float)));
  }
  // outside the image: the ordinary fold (K0) of the channel mean, into every constants image as asdf_decoder_set_sample does
  hipLaunchKernelGGL(channel_mean_kernel, dim3(C), dim3(64), 0, st, feat_dev, H, W, d->pa_lat);
  ASDF_HIP(hipGetLastError());
  ASDF_TRY(set_sample_fold(d, d->pa_lat, st));
  // inside: the biases (the same fold with a zero latent) and P = W_lat . F of both heads and both latent-carrying layers
  FoldParams fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.wlat = d->wlat; fp.wpt = d->wpt; fp.bias02 = d->bias02; fp.embed = d->embed; fp.latent = d->pa_lat + kLatent;
  fp.kp = d->kp;
  fp.cst[0] = d->pa_cstb;
  for (int h = 0; h < kHeads; ++h) {
    fp.pf[h] = d->spec.point_feats[h];
    for (int i = 0; i < 3; ++i) { fp.s2[i][h] = 1.0f; fp.s0[i][h] = 1.0f; }
  }
  hipLaunchKernelGGL(fold_sample_kernel, dim3(kHeads * 2 * kHidden / 4, 1), dim3(256), 0, st, fp);
  hipLaunchKernelGGL(pixel_project_kernel, dim3((unsigned)((hw + 63) / 64), kHidden / 64, kHeads * 2), dim3(256), 0, st, d->wlat, feat_dev,
                     (int)hw, d->pa_proj);
  ASDF_HIP(hipGetLastError());
  PixelParams& q = d->pixel;
  q.proj = d->pa_proj; q.cstb = d->pa_cstb; q.ws = d->pa_ws;
  for (int i = 0; i < 12; ++i) q.cam[i] = cam3x4[i];
  for (int i = 0; i < 3; ++i) q.root[i] = root3[i];
  q.image_size = image_size; q.scale = scale_factor; q.H = H; q.W = W;
  d->pixel_bound = true;
  return ASDF_OK;
}

int asdf_decode_grid(asdf_decoder_t* d, int32_t N, const float origin[3], float voxel_size, int32_t grid_mode,
                     float* sdf_hand_dev, float* sdf_obj_dev, int32_t* bbox_dev, void* stream) {
  if (!origin) return ASDF_EINVAL;
  return decode_grid_impl(d, N, origin, voxel_size, nullptr, grid_mode, sdf_hand_dev, sdf_obj_dev, bbox_dev, stream);
}

int asdf_decode_grid_dev(asdf_decoder_t* d, int32_t N, const float* lattice_dev, int32_t grid_mode,
                         float* sdf_hand_dev, float* sdf_obj_dev, int32_t* bbox_dev, void* stream) {
  if (!lattice_dev) return ASDF_EINVAL;
  return decode_grid_impl(d, N, nullptr, 0.0f, lattice_dev, grid_mode, sdf_hand_dev, sdf_obj_dev, bbox_dev, stream);
}

int asdf_zoom_cube(const int32_t* bbox_dev, int32_t N, float voxel_size, int32_t hand_branch, int32_t obj_branch, float* lattice_dev,
                   void* stream) {
  if (!bbox_dev || !lattice_dev || N < 2 || (!hand_branch && !obj_branch)) return ASDF_EINVAL;
  hipLaunchKernelGGL(zoom_cube_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, bbox_dev, N, voxel_size, hand_branch, obj_branch, lattice_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_decode_grid_box(asdf_decoder_t* d, int32_t N, const float origin[3], float voxel_size, int32_t grid_mode, float tau,
                         float* scratch_hand_dev, float* scratch_obj_dev, int32_t* bbox_dev, void* stream) {
  if (!origin) return ASDF_EINVAL;
  DecodeParams p;
  ASDF_TRY(one_plane_params(d, N, origin, voxel_size, nullptr, grid_mode, tau, scratch_hand_dev, scratch_obj_dev, bbox_dev, p));
  const bool two_out = d->spec.num_heads == 1;
  hipStream_t st = (hipStream_t)stream;
  p.neg_thr = -tau;                                                   // the fused box takes the CERTAINLY negative voxels
  // (cleared with the record: the candidate count and the audit pick count)
  ASDF_TRY(one_plane_sweep(d, p, ClearRange{d->near_count, 1}, ClearRange{d->audit_count, 1}, st));
  // audit: voxels both heads decided by sign alone, drawn at random, through the split-half kernel (the arithmetic of the
  // ordinary sweep) - they report the error of the one-plane values where nothing else looks.  The picks are drawn here, in
  // order; their evaluation (a latency-bound launch on the small lattices: one 128-point tile per compute unit or less) runs on
  // the decoder's audit stream beside the candidates below - it reads the volume at the picks (never candidates: |v| >= tau) and
  // writes only the audit record, which nothing reads before the join in front of sweep_record_kernel
  bool audit_forked = false;
  // (a scope guard: whichever way this function is left behind the fork - an ASDF_HIP early return, a failed launch_subset - the
  // caller's stream waits for the audit's kernels, so the next call's sweep_init_kernel cannot clear the audit record under them:
  // ADVICE r05)
  struct AuditJoin {
    asdf_decoder* d; hipStream_t st; const bool* forked; bool done = false;
    void join() { if (*forked && !done) { done = true; (void)hipStreamWaitEvent(st, d->ev_audit_join, 0); } }
    ~AuditJoin() { join(); }
  } audit_join{d, st, &audit_forked};
  if (d->audit_n > 0) {
    ASDF_TRY(enqueue_audit_picks(d, p.sdf0, p.sdf1, nullptr, p.P, tau, d->audit_idx, d->audit_count, kAuditCap, 0, st));
    int agrid;
    DecodeParams a = list_params(d, p, d->stream16, d->cst16, d->audit_idx, d->audit_count, kAuditCap, &agrid);
    a.bbox = nullptr; a.neg_thr = 0.0f;
    a.audit = d->audit_rec; a.audit_from = nullptr;
    hipStream_t as = st;
    if (d->audit_side && !std::getenv("ASDF_AUDIT_INLINE")) {
      ASDF_HIP(hipEventRecord(d->ev_audit_fork, st));
      ASDF_HIP(hipStreamWaitEvent(d->audit_side, d->ev_audit_fork, 0));
      as = d->audit_side;
      audit_forked = true;
    }
    k1h_subset_launch(d->kp, two_out, a, agrid, as);
    if (audit_forked && hipEventRecord(d->ev_audit_join, d->audit_side) != hipSuccess) {
      // no event to wait for: drain the side stream here, then report
      (void)hipStreamSynchronize(d->audit_side);
      audit_forked = false;
      return ASDF_EHIP;
    }
  }
  // candidates -> exact values (fp32 MFMA chain) -> the box is extended by every candidate that is negative
  const long long items = (N & 3) == 0 ? p.P / 4 : p.P;
  const int cgrid = (int)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);
  // A lattice of up to 8 x kCandDirect voxels (N <= 64) gets no two-step form: more than kCandDirect candidates there would mean an
  // eighth of the lattice within tau of the level - such a sweep is refused as a list overflow (ASDF_STATUS_LIST_OVERFLOW, the caller repeats it as an
  // ordinary sweep) and its five launches, which did nothing in every other sweep, are not enqueued (a 64^3 sample is ~40 launches)
  const bool direct_only = p.P <= 8LL * kCandDirect;
  const int cand_cap = direct_only ? kCandDirect : kCandCap;
  hipLaunchKernelGGL(collect_box_candidates_kernel, dim3(cgrid), dim3(256), 0, st, p.sdf0, p.sdf1, N, tau, p.bbox, d->near_idx,
                     d->near_count, cand_cap, d->status);
  if (!d->box_aux) ASDF_HIP(hipMalloc((void**)&d->box_aux, (4 + (size_t)kNearCap) * sizeof(int)));
  int* direct_count = d->box_aux, *twostep_count = d->box_aux + 1, *twostep_near = d->box_aux + 2, *twostep_idx = d->box_aux + 4;
  hipLaunchKernelGGL(split_candidate_count_kernel, dim3(1), dim3(64), 0, st, d->near_count, cand_cap, kCandDirect, d->box_aux);
  int rgrid;
  {
    // up to kCandDirect candidates: the fp32 chain patches values and boxes in one step
    DecodeParams q = list_params(d, p, d->stream, d->cst, d->near_idx, direct_count, kCandCap, &rgrid);
    q.fixup_flag = d->status + ASDF_STATUS_FIXUP;
    ASDF_TRY(launch_subset(d, q, two_out, rgrid, st));
  }
  if (!direct_only) {
    // more: the values of the ordinary sweep (split-half kernel; it reports the largest |exact - one-plane| to ASDF_STATUS_MAX_ERR) ...
    DecodeParams e = list_params(d, p, d->stream16, d->cst16, d->near_idx, twostep_count, kCandCap, &rgrid);
    e.bbox = nullptr; e.neg_thr = 0.0f;
    k1h_subset_launch(d->kp, two_out, e, rgrid, st);
    if (d->refine_tau > 0.0f) {
      // ... the fp32 chain where they lie within refine_tau of the level ...
      const float* vols[2] = {p.sdf0, p.sdf1};
      for (int h = 0; h < 2; ++h)
        if (vols[h])
          hipLaunchKernelGGL(collect_near_level_list_kernel, dim3(256), dim3(256), 0, st, vols[h], d->near_idx, twostep_count, kCandCap,
                             d->refine_tau, twostep_idx, twostep_near, kNearCap, d->status);
      int ngrid;
      DecodeParams f = list_params(d, p, d->stream, d->cst, twostep_idx, twostep_near, kNearCap, &ngrid);
      f.bbox = nullptr; f.neg_thr = 0.0f; f.status = nullptr;
      ASDF_TRY(launch_subset(d, f, two_out, ngrid, st));
    }
    // ... and the boxes take every candidate that is negative
    hipLaunchKernelGGL(extend_box_from_list_kernel, dim3(256), dim3(256), 0, st, p.sdf0, p.sdf1, d->near_idx, twostep_count, N, p.bbox);
  }
  // the record of this call travels with the boxes: one read-back for the caller
  audit_join.join();
  hipLaunchKernelGGL(sweep_record_kernel, dim3(1), dim3(64), 0, st, bbox_dev, d->status, d->near_count, d->audit_rec);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_decode_grid_band(asdf_decoder_t* d, int32_t N, const float origin[3], float voxel_size, int32_t grid_mode, float tau,
                          float* sdf_hand_dev, float* sdf_obj_dev, int32_t* rec_dev, void* stream) {
  if (!origin) return ASDF_EINVAL;
  return decode_grid_band_impl(d, N, origin, voxel_size, nullptr, grid_mode, tau, sdf_hand_dev, sdf_obj_dev, rec_dev, stream);
}

int asdf_decode_grid_band_dev(asdf_decoder_t* d, int32_t N, const float* lattice_dev, int32_t grid_mode, float tau,
                              float* sdf_hand_dev, float* sdf_obj_dev, int32_t* rec_dev, void* stream) {
  if (!lattice_dev) return ASDF_EINVAL;
  return decode_grid_band_impl(d, N, nullptr, 0.0f, lattice_dev, grid_mode, tau, sdf_hand_dev, sdf_obj_dev, rec_dev, stream);
}

int asdf_decoder_one_plane_usable(const asdf_decoder_t* d) { return d && d->stream16_hi && d->p1_usable ? 1 : 0; }

int asdf_decoder_set_short_list(asdf_decoder_t* d, int32_t max_points) {
  if (!d || max_points < 0 || max_points > (1 << 16)) return ASDF_EINVAL;
  d->short_max = max_points;
  return ASDF_OK;
}

int asdf_decoder_set_cluster_list(asdf_decoder_t* d, int32_t max_points) {
  if (!d || max_points < 0 || max_points > kClusterCap) return ASDF_EINVAL;
  d->shortp.cluster_max = max_points;
  // switching the form (back) on withdraws an earlier fault report (ASDF_STATUS_CLUSTER_FAULT is sticky otherwise: asdf_decoder_status leaves it)
  if (max_points > 0 && d->shortp.fault) { ASDF_HIP(hipDeviceSynchronize()); ASDF_HIP(hipMemset(d->shortp.fault, 0, sizeof(int))); }
  return ASDF_OK;
}

int asdf_decoder_set_cluster_timeout(asdf_decoder_t* d, uint64_t ticks) {
  if (!d) return ASDF_EINVAL;
  d->shortp.timeout_ticks = ticks ? ticks : kClusterTimeoutTicks;
  return ASDF_OK;
}

int asdf_decoder_set_audit(asdf_decoder_t* d, int32_t voxels, uint64_t seed) {
  if (!d || voxels < 0 || voxels > kAuditCap) return ASDF_EINVAL;
  d->audit_n = voxels;
  d->audit_seed = seed;
  return ASDF_OK;
}

int asdf_decode_points(asdf_decoder_t* d, const float* xyz_dev, int64_t M, float* sdf_hand_dev, float* sdf_obj_dev,
                       void* stream) {
  if (!d || M < 0 || (M > 0 && !xyz_dev)) return ASDF_EINVAL;
  DecodeParams p;
  std::memset(&p, 0, sizeof(p));
  p.sdf0 = sdf_hand_dev; p.sdf1 = sdf_obj_dev; p.xyz = xyz_dev; p.P = M; p.N = 1; p.mode = kPointList;
  return launch_decode(d, p, (hipStream_t)stream);
}

int asdf_decode_points_grad(asdf_decoder_t* d, const float* xyz_dev, int64_t M, float* sdf_hand_dev, float* grad_hand_dev,
                            float* sdf_obj_dev, float* grad_obj_dev, void* stream) {
  if (!d || M < 0 || (M > 0 && !xyz_dev)) return ASDF_EINVAL;
  if (!d->sample_bound) return ASDF_EINVAL;
  if (!point_list_covered(d)) return ASDF_ENOGRAD;
  const bool want0 = sdf_hand_dev || grad_hand_dev, want1 = sdf_obj_dev || grad_obj_dev;
  if (M == 0 || (!want0 && !want1)) return ASDF_OK;
  hipStream_t st = (hipStream_t)stream;
  DecodeParams p = point_list_params(d, d->cst, xyz_dev, M, (want0 ? 1 : 0) | (want1 ? 2 : 0));
  p.sdf0 = sdf_hand_dev; p.sdf1 = sdf_obj_dev;
  GradParams g;
  g.grad0 = grad_hand_dev; g.grad1 = grad_obj_dev;
  k1g_launch(p, g, k1g_grid(M, d->num_cus), st);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

// the reverse-mode scratch (first use; sized for the largest grid, so no call allocates after it): the workgroups' partial sums
// [num_cus][kVjpFoldFloats], one d_fold block for callers that pass none, the loss form's [num_cus][heads] fp64 sums and, each on a
// 256-byte boundary behind them, asdf_fit_code's sample descriptor and workgroup map [num_cus]
static_assert(sizeof(FitSampleDesc) <= 256, "the workgroup map lies 256 bytes behind the descriptor");
static size_t vjp_scratch_desc_at(const asdf_decoder* d) {
  const size_t sums = ((size_t)d->num_cus + 1) * kVjpFoldFloats * sizeof(float) + (size_t)d->num_cus * kHeads * sizeof(double);
  return (sums + 255) & ~(size_t)255;
}
static int vjp_scratch(asdf_decoder* d) {
  if (d->vjp_partial) return ASDF_OK;
  const size_t bytes = vjp_scratch_desc_at(d) + 256 + (size_t)d->num_cus * sizeof(FitWg);
  const hipError_t e = hipMalloc((void**)&d->vjp_partial, bytes);
  if (e != hipSuccess) { g_last_hip_error = (int)e; d->vjp_partial = nullptr; return e == hipErrorOutOfMemory ? ASDF_ENOMEM : ASDF_EHIP; }
  return ASDF_OK;
}

int asdf_decode_points_vjp(asdf_decoder_t* d, const float* xyz_dev, int64_t M, const float* w_hand_dev, const float* w_obj_dev,
                           float* sdf_hand_dev, float* sdf_obj_dev, float* d_fold_dev, float* d_latent_dev, float* d_embed_dev, void* stream) {
  if (!d || M < 0 || (M > 0 && !xyz_dev)) return ASDF_EINVAL;
  if (!d->sample_bound) return ASDF_EINVAL;
  if (!point_list_covered(d) || !d->streamT) return ASDF_ENOGRAD;
  hipStream_t st = (hipStream_t)stream;
  const int heads_mask = (w_hand_dev ? 1 : 0) | (w_obj_dev ? 2 : 0);
  if (M == 0 || !heads_mask) {
    if (d_fold_dev) ASDF_HIP(hipMemsetAsync(d_fold_dev, 0, kVjpFoldFloats * sizeof(float), st));
    if (d_latent_dev) ASDF_HIP(hipMemsetAsync(d_latent_dev, 0, kLatent * sizeof(float), st));
    if (d_embed_dev) ASDF_HIP(hipMemsetAsync(d_embed_dev, 0, (size_t)kHeads * ASDF_MAX_POINT_FEATS * 4 * sizeof(float), st));
    return ASDF_OK;
  }
  ASDF_TRY(vjp_scratch(d));
  DecodeParams p = point_list_params(d, d->cst, xyz_dev, M, heads_mask);
  p.sdf0 = w_hand_dev ? sdf_hand_dev : nullptr; p.sdf1 = w_obj_dev ? sdf_obj_dev : nullptr;
  VjpParams v;
  v.streamT = d->streamT; v.w[0] = w_hand_dev; v.w[1] = w_obj_dev; v.partial = d->vjp_partial;
  const int grid = k1v_grid(M, d->num_cus);
  k1v_launch(p, v, grid, st);
  float* fold = d_fold_dev ? d_fold_dev : d->vjp_partial + (size_t)d->num_cus * kVjpFoldFloats;
  k1v_finish(d->vjp_partial, grid, heads_mask, fold, d->wlat, d->wpt, ASDF_MAX_POINT_FEATS, d_latent_dev, d_embed_dev, st);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

// The batch of one on the decoder's own memory: its constants images (the fold is set_sample's, so the sample stays bound to the moving
// code in every image and the status word counts as ever), its reverse-mode scratch, and the caller's state buffer.
int asdf_fit_code(asdf_decoder_t* d, const float* xyz_dev, int64_t M, const float* t_hand_dev, int32_t n_hand, const float* t_obj_dev,
                  int32_t n_obj, float clamp, float* z_dev, const float* z0_dev, float prior, const float* step_table_dev, int32_t steps,
                  void* state_dev, size_t state_bytes, double* history_dev, void* stream) {
  if (!d || M < 0 || steps < 0 || n_hand < 0 || n_obj < 0 || (M > 0 && !xyz_dev)) return ASDF_EINVAL;
  if (!d->sample_bound) return ASDF_EINVAL;
  if (!point_list_covered(d) || !d->streamT) return ASDF_ENOGRAD;
  if (steps == 0 || M == 0) return ASDF_OK;
  if (!z_dev || !step_table_dev || !state_dev || state_bytes < ASDF_FIT_STATE_BYTES || ((uintptr_t)state_dev & 3)) return ASDF_EINVAL;
  if (!(clamp > 0.0f) || !(prior >= 0.0f) || n_hand > M || n_obj > M || M > INT32_MAX) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  ASDF_TRY(vjp_scratch(d));
  const FitSampleDesc desc = fit_describe(d, 0, M, 0, t_hand_dev ? n_hand : 0, t_obj_dev ? n_obj : 0);
  char* tail = reinterpret_cast<char*>(d->vjp_partial) + vjp_scratch_desc_at(d);
  FitBuffers b;
  b.samples = reinterpret_cast<FitSampleDesc*>(tail);
  b.wgs = reinterpret_cast<FitWg*>(tail + 256);
  b.cst = d->cst;
  b.partial = d->vjp_partial;
  b.fold = d->vjp_partial + (size_t)d->num_cus * kVjpFoldFloats;
  b.loss_partial = reinterpret_cast<double*>(d->vjp_partial + ((size_t)d->num_cus + 1) * kVjpFoldFloats);
  b.state = static_cast<float*>(state_dev);
  b.xyz = xyz_dev; b.t[0] = t_hand_dev; b.t[1] = t_obj_dev;
  b.z = z_dev; b.z0 = z0_dev; b.step_table = step_table_dev; b.history = history_dev;
  ASDF_TRY(fit_loop(d, &desc, 1, b, clamp, prior, steps, st, [&] { return set_sample_fold(d, z_dev, st); }));
  return set_sample_fold(d, z_dev, st);
}

// asdf_fit_codes' workspace, every part 256-byte aligned: [descriptors | workgroup map | constants blocks | partial sums | d_fold |
// loss partials | Adam states].  ASDF_EINVAL where the batch cannot be described (the descriptors' words are 32-bit).
struct FitCodesLayout {
  size_t samples, wgs, cst, partial, fold, loss, state, bytes;
};
static int fit_codes_layout(const asdf_decoder* d, int32_t B, const int64_t* m, FitCodesLayout* L) {
  if (!d || !m || !L || B < 1 || B > 65535) return ASDF_EINVAL;
  long long pts = 0, wgs = 0;
  for (int s = 0; s < B; ++s) {
    if (m[s] < 1 || m[s] > INT32_MAX) return ASDF_EINVAL;
    pts += m[s];
    wgs += k1v_grid(m[s], d->num_cus);
  }
  if (pts > INT32_MAX || wgs > INT32_MAX) return ASDF_EINVAL;
  size_t at = 0;
  auto part = [&](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
  L->samples = part((size_t)B * sizeof(FitSampleDesc));
  L->wgs = part((size_t)wgs * sizeof(FitWg));
  L->cst = part((size_t)B * kHeads * kCstFloats * sizeof(float));
  L->partial = part((size_t)wgs * kVjpFoldFloats * sizeof(float));
  L->fold = part((size_t)B * kVjpFoldFloats * sizeof(float));
  L->loss = part((size_t)wgs * kHeads * sizeof(double));
  L->state = part((size_t)B * kFitStateFloats * sizeof(float));
  L->bytes = at;
  return ASDF_OK;
}

int asdf_fit_codes_workspace_bytes(const asdf_decoder_t* d, int32_t B, const int64_t* m, size_t* bytes) {
  if (!bytes) return ASDF_EINVAL;
  FitCodesLayout L;
  ASDF_TRY(fit_codes_layout(d, B, m, &L));
  *bytes = L.bytes;
  return ASDF_OK;
}

int asdf_fit_codes(asdf_decoder_t* d, int32_t B, const float* xyz_dev, const int64_t* m, const float* t_hand_dev, const int32_t* n_hand,
                   const float* t_obj_dev, const int32_t* n_obj, float clamp, float* z_dev, const float* z0_dev, const float* embed_dev,
                   float prior, const float* step_table_dev, int32_t steps, void* workspace_dev, size_t workspace_bytes,
                   double* history_dev, void* stream) {
  if (!d || B < 1 || steps < 0 || !m || !xyz_dev) return ASDF_EINVAL;
  if (!point_list_covered(d) || !d->streamT) return ASDF_ENOGRAD;
  if (steps == 0) return ASDF_OK;
  if (!z_dev || !embed_dev || !step_table_dev || !workspace_dev || ((uintptr_t)workspace_dev & 15)) return ASDF_EINVAL;
  if (!(clamp > 0.0f) || !(prior >= 0.0f) || (t_hand_dev && !n_hand) || (t_obj_dev && !n_obj)) return ASDF_EINVAL;
  FitCodesLayout L;
  ASDF_TRY(fit_codes_layout(d, B, m, &L));
  if (workspace_bytes < L.bytes) return ASDF_EINVAL;
  std::vector<FitSampleDesc> descs((size_t)B);
  int first = 0, wg0 = 0;
  for (int s = 0; s < B; ++s) {
    const int64_t nh = t_hand_dev ? n_hand[s] : 0, no = t_obj_dev ? n_obj[s] : 0;
    if (nh < 0 || no < 0 || nh > m[s] || no > m[s] || (nh == 0 && no == 0)) return ASDF_EINVAL;
    descs[(size_t)s] = fit_describe(d, first, m[s], wg0, nh, no);
    first += descs[(size_t)s].m; wg0 += descs[(size_t)s].grid;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  float* cst_all = reinterpret_cast<float*>(ws + L.cst);
  // the constants come from the workspace, so neither the bound sample nor any image of the decoder is touched
  FitBuffers b;
  b.samples = reinterpret_cast<FitSampleDesc*>(ws + L.samples);
  b.wgs = reinterpret_cast<FitWg*>(ws + L.wgs);
  b.cst = cst_all;
  b.partial = reinterpret_cast<float*>(ws + L.partial);
  b.fold = reinterpret_cast<float*>(ws + L.fold);
  b.loss_partial = reinterpret_cast<double*>(ws + L.loss);
  b.state = reinterpret_cast<float*>(ws + L.state);
  b.xyz = xyz_dev; b.t[0] = t_hand_dev; b.t[1] = t_obj_dev;
  b.z = z_dev; b.z0 = z0_dev; b.step_table = step_table_dev; b.history = history_dev;
  FoldParams fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.wlat = d->wlat; fp.wpt = d->wpt; fp.bias02 = d->bias02; fp.kp = d->kp;
  for (int h = 0; h < kHeads; ++h) {
    fp.pf[h] = d->spec.point_feats[h];
    for (int i = 0; i < 3; ++i) { fp.s2[i][h] = 1.0f; fp.s0[i][h] = 1.0f; }
  }
  k1vb_cst_init(d->cst, cst_all, B, st);
  return fit_loop(d, descs.data(), B, b, clamp, prior, steps, st, [&] { k1vb_fold(fp, z_dev, embed_dev, cst_all, B, st); return ASDF_OK; });
}

int asdf_trace_rays(asdf_decoder_t* d, const float* rays_dev, int64_t M, const asdf_trace_params_t* params,
                    float* t_hand_dev, int32_t* status_hand_dev, float* bracket_hand_dev, int32_t* evals_hand_dev,
                    float* t_obj_dev, int32_t* status_obj_dev, float* bracket_obj_dev, int32_t* evals_obj_dev, void* stream) {
  if (!d || M < 0 || !params || (M > 0 && !rays_dev)) return ASDF_EINVAL;
  if (!d->sample_bound) return ASDF_EINVAL;
  if (params->max_steps < 1 || params->refine_steps < 0 || !(params->min_step > 0.0f) || !(params->max_step > 0.0f)) return ASDF_EINVAL;
  // (the kernel moves a ray and a bracket as one 16-byte word each)
  if (((uintptr_t)rays_dev | (uintptr_t)bracket_hand_dev | (uintptr_t)bracket_obj_dev) & 15) return ASDF_EINVAL;
  if (!point_list_covered(d)) return ASDF_ENOTRACE;
  const bool want0 = t_hand_dev || status_hand_dev, want1 = t_obj_dev || status_obj_dev;
  if (M == 0 || (!want0 && !want1)) return ASDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const DecodeParams p = point_list_params(d, d->cst, nullptr, M, (want0 ? 1 : 0) | (want1 ? 2 : 0));
  TraceParams q;
  std::memset(&q, 0, sizeof(q));
  q.rays = rays_dev; q.M = M;
  q.rule = TraceRule{params->max_steps, params->refine_steps, params->step_scale, params->min_step, params->max_step};
  q.out[0] = TraceOutputs{t_hand_dev, status_hand_dev, bracket_hand_dev, evals_hand_dev};
  q.out[1] = TraceOutputs{t_obj_dev, status_obj_dev, bracket_obj_dev, evals_obj_dev};
  q.queue = d->trace_queue;
  ASDF_HIP(hipMemsetAsync(d->trace_queue, 0, 2 * sizeof(unsigned long long), st));
  k1t_launch(p, q, k1t_grid(M, d->num_cus), st);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_project_points(asdf_decoder_t* d, const float* xyz_dev, int64_t M, int32_t head, const asdf_project_params_t* params,
                        float* xyz_out_dev, float* sdf_dev, float* grad_dev, float* sdf_in_dev, int32_t* status_dev, int32_t* evals_dev,
                        void* stream) {
  if (!d || M < 0 || (M > 0 && !xyz_dev) || !params) return ASDF_EINVAL;
  if (!d->sample_bound) return ASDF_EINVAL;
  if (params->max_iters < 0 || !(params->tol >= 0.0f) || !(params->max_move > 0.0f) || !(params->min_grad2 > 0.0f)) return ASDF_EINVAL;
  if (!point_list_covered(d)) return ASDF_ENOPROJECT;
  if (head < 0 || head >= d->spec.num_heads) return ASDF_EINVAL;
  if (M == 0) return ASDF_OK;
  if (!xyz_out_dev && !sdf_dev && !grad_dev && !sdf_in_dev && !status_dev && !evals_dev) return ASDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const DecodeParams p = point_list_params(d, d->cst, xyz_dev, M, 1 << head);
  ProjectParams q;
  std::memset(&q, 0, sizeof(q));
  q.rule = ProjectRule{params->max_iters, params->tol, params->max_move, params->min_grad2};
  q.xyz_out = xyz_out_dev; q.sdf = sdf_dev; q.grad = grad_dev; q.sdf_in = sdf_in_dev; q.status = status_dev; q.evals = evals_dev;
  k1p_launch(p, q, k1p_grid(M, d->num_cus), st);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_decoder_set_math(asdf_decoder_t* d, int32_t math) {
  if (!d || (math != ASDF_MATH_F32 && math != ASDF_MATH_F16X3)) return ASDF_EINVAL;
  if (math == ASDF_MATH_F16X3 && (!d->stream16 || d->pixel_bound)) return ASDF_EINVAL;
  d->math = math;
  return ASDF_OK;
}

int asdf_decoder_get_math(const asdf_decoder_t* d) { return d ? d->math : ASDF_EINVAL; }

int asdf_decoder_time_next_sweep(asdf_decoder_t* d, void* event_start, void* event_stop) {
  if (!d || (!event_start) != (!event_stop)) return ASDF_EINVAL;
  d->ev_start = event_start;
  d->ev_stop = event_stop;
  return ASDF_OK;
}

int asdf_decoder_set_refine(asdf_decoder_t* d, float tau) {
  if (!d || !(tau >= 0.0f) || tau > 1.0f) return ASDF_EINVAL;
  d->refine_tau = tau;
  return ASDF_OK;
}

int asdf_decoder_status(asdf_decoder_t* d, int32_t out_host[16], int32_t clear, void* stream) {
  if (!d || !out_host) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  ASDF_HIP(hipMemcpyAsync(out_host, d->status, ASDF_STATUS_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
  if (clear) {       // (the cluster form's fault report is sticky: asdf_decoder_set_cluster_list withdraws it)
    ASDF_HIP(hipMemsetAsync(d->status, 0, ASDF_STATUS_CLUSTER_FAULT * sizeof(int), st));
    ASDF_HIP(hipMemsetAsync(d->status + ASDF_STATUS_CLUSTER_FAULT + 1, 0, (ASDF_STATUS_WORDS - ASDF_STATUS_CLUSTER_FAULT - 1) * sizeof(int), st));
  }
  ASDF_HIP(hipStreamSynchronize(st));
  return ASDF_OK;
}

int asdf_decoder_get_act_scales(const asdf_decoder_t* d, float sx_out[ASDF_MAX_HEADS][3]) {
  if (!d || !sx_out) return ASDF_EINVAL;
  std::memcpy(sx_out, d->sx, sizeof(d->sx));
  return ASDF_OK;
}

int asdf_decoder_set_act_scales(asdf_decoder_t* d, const float sx[ASDF_MAX_HEADS][3], void* stream) {
  if (!d || !sx || !d->cst16) return ASDF_EINVAL;
  for (int h = 0; h < d->spec.num_heads; ++h)
    for (int l = 0; l < 3; ++l) {
      int e = 0;
      const float m = std::frexp(sx[h][l], &e);
      if (!(sx[h][l] > 0.0f) || m != 0.5f || e < -23 || e > 25) return ASDF_EINVAL;      // powers of two in [2^-24, 2^24]
    }
  hipStream_t st = (hipStream_t)stream;
  ASDF_HIP(hipStreamSynchronize(st));                      // sweeps in flight still read the old constants
  std::memcpy(d->sx, sx, sizeof(d->sx));
  const size_t n = (size_t)kHeads * cst_offsets(d->kp).floats;
  std::memcpy(d->cst16_host, d->cst_host, n * sizeof(float));
  scale_constants_f16(d->spec, d->kp, d->cst_host, d->sw, d->sx, d->cst16_host, d->s2);
  ASDF_HIP(hipMemcpy(d->cst16, d->cst16_host, n * sizeof(float), hipMemcpyHostToDevice));
  ASDF_HIP(rebuild_one_plane(d));
  d->sample_bound = false;                                 // the folded per-sample constants carried the old layer-2 scale
  return ASDF_OK;
}

int asdf_debug_grid_coords(int32_t N, const float origin[3], float voxel_size, int32_t grid_mode, int64_t first, int64_t count,
                           float* coords_dev, void* stream) {
  if (!origin || !coords_dev || N < 2 || N > 1024 || first < 0 || count < 0 || first + count > (int64_t)N * N * N) return ASDF_EINVAL;
  if (grid_mode != ASDF_GRID_REFERENCE && grid_mode != ASDF_GRID_INTEGER) return ASDF_EINVAL;
  if (count == 0) return ASDF_OK;
  hipLaunchKernelGGL(grid_coords_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coords_dev,
                     (long long)first, (long long)count, N, grid_mode == ASDF_GRID_REFERENCE ? kGridReference : kGridInteger,
                     voxel_size, origin[0], origin[1], origin[2]);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_decoder_set_classifier(asdf_decoder_t* d, const float* w_host, const float* b_host, int32_t num_class) {
  if (!d || !w_host || !b_host || num_class < 1 || num_class > kMaxClasses) return ASDF_EINVAL;
  std::vector<float> img(kClsFloats, 0.0f);
  for (int k = 0; k < num_class; ++k) {
    for (int row = 0; row < kHidden; ++row) {
      const int t = row >> 5, rr = row & 31, hh = (rr >> 2) & 1, r = (rr & 3) + 4 * (rr >> 3);   // D-layout order
      img[(size_t)k * kHidden + (t * 2 + hh) * 16 + r] = w_host[(size_t)k * kHidden + row];
    }
    img[(size_t)kMaxClasses * kHidden + k] = b_host[k];
  }
  if (!d->cls) ASDF_HIP(hipMalloc((void**)&d->cls, img.size() * sizeof(float)));
  ASDF_HIP(hipMemcpy(d->cls, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  d->num_class = num_class;
  return ASDF_OK;
}

int asdf_decode_points_cls(asdf_decoder_t* d, const float* xyz_dev, int64_t M, float* sdf_hand_dev, float* sdf_obj_dev,
                           float* logits_dev, int32_t* labels_dev, void* stream) {
  if (!d || M < 0 || (M > 0 && !xyz_dev) || (!logits_dev && !labels_dev)) return ASDF_EINVAL;
  DecodeParams p;
  std::memset(&p, 0, sizeof(p));
  p.sdf0 = sdf_hand_dev; p.sdf1 = sdf_obj_dev; p.xyz = xyz_dev; p.P = M; p.N = 1; p.mode = kPointList;
  p.logits = logits_dev; p.labels = labels_dev;
  return launch_decode(d, p, (hipStream_t)stream);
}

}  // extern "C"
