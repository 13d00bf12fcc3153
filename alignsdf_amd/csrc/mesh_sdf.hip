// Signed distance field of a triangle mesh (include/alignsdf_hip.h: asdf_mesh_sdf_*): exact point-triangle distance by region, sign from
// the generalised winding number.  Plain device arrays, no decoder.  One query per lane; the face is the same for every lane of a
// wave, so its record comes out of LDS as a broadcast and every decision ABOUT THE FACE (absent, zero-area) is a wave-uniform branch.
// Every pair is visited: the winding sum needs every face, so there is no culling here.
//
// Bit-repeatability is by construction: a lane's result is a function of its query and the records alone.  The minimum is exact in any
// grouping (strict <, faces in index order); the winding sum is taken per chunk of kChunk faces from +0 and the chunk sums are added in
// chunk order from +0 - by the wave that walks all chunks, or by the combine kernel over the partials of a split launch.  No atomics
// on results (the two info counters of the prep launch are integer counts).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/alignsdf_hip.h"
#include "common.h"

namespace asdf {
namespace {

constexpr int kWave = 64;                                  // one wave per workgroup: small query lists still spread over the device
constexpr int kBlock = ASDF_MESH_SDF_BLOCK_FACES;          // records staged into LDS at a time
constexpr int kChunk = ASDF_MESH_SDF_CHUNK_FACES;          // the summation unit of the winding number
constexpr int kRecVec = ASDF_MESH_SDF_RECORD_BYTES / 16;   // float4 per record: (a, state), (b, 0), (c, 0)
constexpr int kHeaderVec = 1;                              // int32[4] in front of the records: (faces prepared, kMagic, 0, 0)
constexpr int kMagic = 0x4d534446;
constexpr int kFaceOk = 0, kFaceZeroArea = 1, kFaceAbsent = 2;      // a record's state word, plus
constexpr int kFaceFlipped = 4;                                     // the corners' index order is an odd permutation of the face's
constexpr long long kSplitMaxQueries = ASDF_MESH_SDF_SPLIT_MAX_QUERIES;
constexpr int kSplitWaves = 4096;                          // a split launch aims at this many waves (1024 SIMDs x 4)
constexpr long long kSliceQueries = 1ll << 30;             // queries per launch of the whole shape (grid.x < 2^31 / 64)
constexpr float kTwoPi = 6.28318530717958647692f;

static_assert(kChunk % kBlock == 0 && kRecVec == 3 && (kBlock * kRecVec) % kWave == 0, "whole blocks per chunk, whole trips per block");

constexpr size_t kSplitMaxBytes = 256u << 20;             // scratch a split launch may ask for; beyond it the whole shape runs
constexpr int kMaxFaces = 0x7fffffff - kChunk;             // the padded count still fits an int

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 along(V3 base, float t, V3 e) { return {base.x + t * e.x, base.y + t * e.y, base.z + t * e.z}; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// closest point of the closed triangle (a, b, c) to p: the header's region rule.  The three edge regions share one division.
__device__ __forceinline__ V3 closest_on_triangle(V3 a, V3 b, V3 c, V3 p) {
  const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
  const V3 ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  // (numerator, denominator, base, direction) of the first matching region; a corner is base + (0 / 1) direction
  float num = 0.0f, den = 1.0f;
  V3 base = a, dir = ab;
  bool interior = false;
  if (d1 <= 0.0f && d2 <= 0.0f) { base = a; }
  else if (d3 >= 0.0f && d4 <= d3) { base = b; }
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { num = d1; den = d1 - d3; }
  else if (d6 >= 0.0f && d5 <= d6) { base = c; }
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { num = d2; den = d2 - d6; dir = ac; }
  else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) { num = e43; den = e43 + e56; base = b; dir = bc; }
  else { interior = true; }
  const V3 q_edge = along(base, num / den, dir);
  const float s = (va + vb) + vc;
  const V3 q_in = along(along(a, vb / s, ab), vc / s, ac);
  return interior ? q_in : q_edge;
}

// closest point of the segment base + t e, t in [0, 1]
__device__ __forceinline__ V3 closest_on_segment(V3 base, V3 e, V3 p) {
  const float ee = dot(e, e);
  float t = 0.0f;
  if (ee > 0.0f) t = fminf(fmaxf(dot(sub(p, base), e) / ee, 0.0f), 1.0f);
  return along(base, t, e);
}

// a zero-area face: the nearest of its three edges ab, bc, ca
__device__ __forceinline__ V3 closest_on_flat(V3 a, V3 b, V3 c, V3 p, float* d2_out) {
  V3 q = closest_on_segment(a, sub(b, a), p);
  V3 r = sub(p, q);
  float d2 = dot(r, r);
  const V3 q1 = closest_on_segment(b, sub(c, b), p);
  r = sub(p, q1);
  const float d21 = dot(r, r);
  if (d21 < d2) { d2 = d21; q = q1; }
  const V3 q2 = closest_on_segment(c, sub(a, c), p);
  r = sub(p, q2);
  const float d22 = dot(r, r);
  if (d22 < d2) { d2 = d22; q = q2; }
  *d2_out = d2;
  return q;
}

__device__ __forceinline__ V3 closest_on_face(int state, V3 a, V3 b, V3 c, V3 p, float* d2_out) {
  if (state == kFaceZeroArea) return closest_on_flat(a, b, c, p, d2_out);      // (wave-uniform in the pair loop)
  const V3 q = closest_on_triangle(a, b, c, p);
  const V3 r = sub(p, q);
  *d2_out = dot(r, r);
  return q;
}

// atan2(det, den) of the van Oosterom-Strackee form: half the signed solid angle of (a, b, c) seen from p
__device__ __forceinline__ float half_solid_angle(V3 a, V3 b, V3 c, V3 p) {
  const V3 A = sub(a, p), B = sub(b, p), C = sub(c, p);
  const float la = sqrtf(dot(A, A)), lb = sqrtf(dot(B, B)), lc = sqrtf(dot(C, C));
  const V3 x = {B.y * C.z - B.z * C.y, B.z * C.x - B.x * C.z, B.x * C.y - B.y * C.x};
  const float det = dot(A, x);
  const float den = (((la * lb) * lc + dot(A, B) * lc) + dot(B, C) * la) + dot(C, A) * lb;
  return atan2f(det, den);
}

// faces the kernels may read: what the caller says, never more than what the prep launch wrote (a header that is not one: none)
__device__ __forceinline__ int faces_of(const int4* ws, int num_faces) {
  const int4 h = ws[0];
  return h.y == kMagic ? min(num_faces, max(h.x, 0)) : 0;
}

// ---- prep: one thread per record slot of the padded list
__global__ __launch_bounds__(256) void mesh_sdf_prepare_kernel(const float* __restrict__ verts, int num_verts, const int* __restrict__ faces,
                                                               int num_faces, int slots, float4* __restrict__ ws, int* __restrict__ info) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) reinterpret_cast<int4*>(ws)[0] = make_int4(num_faces, kMagic, 0, 0);
  if (t >= slots) return;
  float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
  if (t < num_faces) {
    int i0 = faces[3 * (long long)t], i1 = faces[3 * (long long)t + 1], i2 = faces[3 * (long long)t + 2];
    int state = kFaceAbsent, flipped = 0;
    // corners in the order of their vertex indices: the distance does not know the face's orientation, the winding term gets its sign
    if (i1 < i0) { const int k = i0; i0 = i1; i1 = k; flipped ^= kFaceFlipped; }
    if (i2 < i1) { const int k = i1; i1 = i2; i2 = k; flipped ^= kFaceFlipped; }
    if (i1 < i0) { const int k = i0; i0 = i1; i1 = k; flipped ^= kFaceFlipped; }
    if ((unsigned)i0 < (unsigned)num_verts && (unsigned)i1 < (unsigned)num_verts && (unsigned)i2 < (unsigned)num_verts) {
      const V3 a = {verts[3 * (long long)i0], verts[3 * (long long)i0 + 1], verts[3 * (long long)i0 + 2]};
      const V3 b = {verts[3 * (long long)i1], verts[3 * (long long)i1 + 1], verts[3 * (long long)i1 + 2]};
      const V3 c = {verts[3 * (long long)i2], verts[3 * (long long)i2 + 1], verts[3 * (long long)i2 + 2]};
      if (finite3(a) && finite3(b) && finite3(c)) {
        const V3 ab = sub(b, a), ac = sub(c, a);
        const float nx = ab.y * ac.z - ab.z * ac.y, ny = ab.z * ac.x - ab.x * ac.z, nz = ab.x * ac.y - ab.y * ac.x;
        state = (nx == 0.0f && ny == 0.0f && nz == 0.0f) ? kFaceZeroArea : kFaceOk;
        r0 = make_float4(a.x, a.y, a.z, 0.0f);
        r1 = make_float4(b.x, b.y, b.z, 0.0f);
        r2 = make_float4(c.x, c.y, c.z, 0.0f);
      }
    }
    r0.w = __int_as_float(state == kFaceOk ? flipped : state);
    if (info && state == kFaceAbsent) atomicAdd(info + ASDF_MESH_SDF_INFO_SKIPPED, 1);
    if (info && state == kFaceZeroArea) atomicAdd(info + ASDF_MESH_SDF_INFO_ZERO_AREA, 1);
  }
  float4* rec = ws + kHeaderVec + (long long)kRecVec * t;
  rec[0] = r0; rec[1] = r1; rec[2] = r2;
}

// ---- the outputs of one query from its reduced state (d2, face, S): shared by both launch shapes
struct Outputs { float* sdf; float* winding; int* face; float* closest; };

__device__ __forceinline__ void finish(const float4* __restrict__ recs, V3 p, float d2, int face, float S, long long q, Outputs o) {
  const float nan = __int_as_float(0x7fc00000);
  float w = S / kTwoPi, d = sqrtf(d2);
  V3 cl = {nan, nan, nan};
  if (!finite3(p)) { w = nan; d = nan; face = -1; }
  if (face >= 0) {
    const float4 r0 = recs[(long long)kRecVec * face], r1 = recs[(long long)kRecVec * face + 1], r2 = recs[(long long)kRecVec * face + 2];
    float again;
    cl = closest_on_face(__float_as_int(r0.w) & 3, {r0.x, r0.y, r0.z}, {r1.x, r1.y, r1.z}, {r2.x, r2.y, r2.z}, p, &again);
  }
  if (o.sdf) o.sdf[q] = fabsf(w) >= 0.5f ? -d : d;
  if (o.winding) o.winding[q] = w;
  if (o.face) o.face[q] = face;
  if (o.closest) { o.closest[3 * q] = cl.x; o.closest[3 * q + 1] = cl.y; o.closest[3 * q + 2] = cl.z; }
}

// ---- the pair kernel.  grid.x: waves of 64 queries; grid.y: groups of `group_chunks` chunks (1 group = the whole shape).
// kSplit: partials to scratch - sums [num_chunks][M] (kWinding), d2 [groups][M], face [groups][M] - else the outputs.
template <bool kWinding, bool kSplit>
__global__ __launch_bounds__(kWave) void mesh_sdf_pair_kernel(const float4* __restrict__ ws, int num_faces, const float* __restrict__ xyz,
                                                              long long M, int num_chunks, int group_chunks, Outputs o,
                                                              float* __restrict__ part_sum, float* __restrict__ part_d2,
                                                              int* __restrict__ part_face) {
  __shared__ float4 s_rec[kBlock * kRecVec];
  const int T = faces_of(reinterpret_cast<const int4*>(ws), num_faces);
  const float4* recs = ws + kHeaderVec;
  const int lane = threadIdx.x;
  const long long q = (long long)blockIdx.x * kWave + lane;
  const bool live = q < M;
  V3 p = {0.0f, 0.0f, 0.0f};
  if (live) p = {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]};
  float best = __int_as_float(0x7f800000), S = 0.0f;
  int best_face = -1;
  const int c0 = kSplit ? blockIdx.y * group_chunks : 0;
  const int c1 = kSplit ? min(c0 + group_chunks, num_chunks) : num_chunks;
  for (int c = c0; c < c1; ++c) {
    float sum = 0.0f;
    const int f1 = min((c + 1) * kChunk, T);                  // (wave-uniform bounds by the REAL count: padding is never looked at)
    for (int f0 = c * kChunk; f0 < f1; f0 += kBlock) {
      __syncthreads();
      // the block's records, 16 bytes per lane and trip (the list is padded to whole chunks: every slot read here was written)
#pragma unroll
      for (int i = 0; i < kBlock * kRecVec / kWave; ++i) s_rec[i * kWave + lane] = recs[(long long)kRecVec * f0 + i * kWave + lane];
      __syncthreads();
      const int n = min(kBlock, f1 - f0);
      for (int j = 0; j < n; ++j) {
        const float4 r0 = s_rec[kRecVec * j], r1 = s_rec[kRecVec * j + 1], r2 = s_rec[kRecVec * j + 2];      // broadcast reads
        const int word = __float_as_int(r0.w), state = word & 3;
        if (state == kFaceAbsent) continue;
        const V3 a = {r0.x, r0.y, r0.z}, b = {r1.x, r1.y, r1.z}, cc = {r2.x, r2.y, r2.z};
        float d2;
        closest_on_face(state, a, b, cc, p, &d2);
        if (d2 < best) { best = d2; best_face = f0 + j; }
        if (kWinding && state == kFaceOk) sum += ((word & kFaceFlipped) ? -1.0f : 1.0f) * half_solid_angle(a, b, cc, p);
      }
    }
    if (kWinding) {
      if (kSplit) { if (live) part_sum[(long long)c * M + q] = sum; }
      else S += sum;
    }
  }
  if (!live) return;
  if (kSplit) {
    part_d2[(long long)blockIdx.y * M + q] = best;
    part_face[(long long)blockIdx.y * M + q] = best_face;
  } else {
    finish(recs, p, best, best_face, S, q, o);
  }
}

// ---- the combine kernel of a split launch: groups in order for the minimum, chunks in order for the sum
template <bool kWinding>
__global__ __launch_bounds__(kWave) void mesh_sdf_combine_kernel(const float4* __restrict__ ws, const float* __restrict__ xyz, long long M,
                                                                 int num_chunks, int groups, Outputs o, const float* __restrict__ part_sum,
                                                                 const float* __restrict__ part_d2, const int* __restrict__ part_face) {
  const long long q = (long long)blockIdx.x * kWave + threadIdx.x;
  if (q >= M) return;
  const V3 p = {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]};
  float best = __int_as_float(0x7f800000), S = 0.0f;
  int best_face = -1;
  for (int g = 0; g < groups; ++g) {
    const float d2 = part_d2[(long long)g * M + q];
    if (d2 < best) { best = d2; best_face = part_face[(long long)g * M + q]; }
  }
  if (kWinding)
    for (int c = 0; c < num_chunks; ++c) S += part_sum[(long long)c * M + q];
  finish(ws + kHeaderVec, p, best, best_face, S, q, o);
}

inline int chunks_of(int num_faces) { return (num_faces + kChunk - 1) / kChunk; }      // (num_faces <= kMaxFaces)

// a split launch: how many chunks a group (one grid.y index) walks, and how many groups that makes
struct SplitPlan { int group_chunks, groups; };
SplitPlan split_plan(int chunks, long long waves) {
  long long want = (kSplitWaves + waves - 1) / waves;
  if (want < 2) want = 2;                                        // (a forced split of a long list still has two groups to reduce)
  if (want > chunks) want = chunks;
  const int group_chunks = (int)((chunks + want - 1) / want);
  return {group_chunks, (chunks + group_chunks - 1) / group_chunks};
}

// scratch of a split launch: sums [chunks][M] fp32, then d2 and face [groups][M]; 0 = this shape is not split (too many queries, or
// it would take more than kSplitMaxBytes: the whole shape gives the same bits)
size_t split_bytes(int num_faces, long long M) {
  const int chunks = chunks_of(num_faces);
  if (M < 1 || M > kSplitMaxQueries || chunks < 1) return 0;
  const SplitPlan plan = split_plan(chunks, (M + kWave - 1) / kWave);
  const unsigned long long bytes = (unsigned long long)M * 4ull * ((unsigned long long)chunks + 2ull * (unsigned long long)plan.groups);
  return bytes > kSplitMaxBytes ? 0 : (size_t)bytes;
}

// the launch shape asked for by the environment variable ASDF_MESH_SDF_SHAPE (read at every call: tests and measurements switch it
// within a process): unset, empty or "auto" = the heuristic, "whole", "split"; anything else = -1
int shape_from_env() {
  const char* v = std::getenv("ASDF_MESH_SDF_SHAPE");
  if (!v || !*v || !std::strcmp(v, "auto")) return ASDF_MESH_SDF_SHAPE_AUTO;
  if (!std::strcmp(v, "whole")) return ASDF_MESH_SDF_SHAPE_WHOLE;
  if (!std::strcmp(v, "split")) return ASDF_MESH_SDF_SHAPE_SPLIT;
  return -1;
}

}  // namespace
}  // namespace asdf

using namespace asdf;

extern "C" {

int asdf_mesh_sdf_workspace_bytes(int32_t num_faces, int64_t M, size_t* bytes) {
  if (!bytes || num_faces < 0 || num_faces > kMaxFaces || M < 0) return ASDF_EINVAL;
  if (M == 0) {
    *bytes = 16 * ((size_t)kHeaderVec + (size_t)kRecVec * kChunk * (size_t)chunks_of(num_faces));
    return ASDF_OK;
  }
  const size_t b = split_bytes(num_faces, M);
  *bytes = b < 16 ? 16 : b;
  return ASDF_OK;
}

int asdf_mesh_sdf_prepare(const float* verts_dev, int32_t num_verts, const int32_t* faces_dev, int32_t num_faces, void* workspace_dev,
                          int32_t* info_dev, void* stream) {
  if (num_verts < 0 || num_faces < 0 || num_faces > kMaxFaces || !workspace_dev || ((uintptr_t)workspace_dev & 15)) return ASDF_EINVAL;
  if ((num_faces > 0 && !faces_dev) || (num_verts > 0 && !verts_dev)) return ASDF_EINVAL;
  if (((uintptr_t)verts_dev | (uintptr_t)faces_dev | (uintptr_t)info_dev) & 3) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (info_dev) ASDF_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * ASDF_MESH_SDF_INFO_WORDS, st));
  const int slots = chunks_of(num_faces) * kChunk;
  const int grid = slots > 0 ? (slots + 255) / 256 : 1;          // (no face: the header alone)
  hipLaunchKernelGGL(mesh_sdf_prepare_kernel, dim3(grid), dim3(256), 0, st, verts_dev, (int)num_verts, (const int*)faces_dev, (int)num_faces,
                     slots, reinterpret_cast<float4*>(workspace_dev), (int*)info_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_mesh_sdf_points(const void* workspace_dev, int32_t num_faces, const float* xyz_dev, int64_t M, float* sdf_dev, float* winding_dev,
                         int32_t* face_dev, float* closest_dev, void* scratch_dev, void* stream) {
  if (num_faces < 0 || num_faces > kMaxFaces || M < 0 || !workspace_dev || ((uintptr_t)workspace_dev & 15) || (M > 0 && !xyz_dev))
    return ASDF_EINVAL;
  if (((uintptr_t)xyz_dev | (uintptr_t)sdf_dev | (uintptr_t)winding_dev | (uintptr_t)face_dev | (uintptr_t)closest_dev |
       (uintptr_t)scratch_dev) & 3)
    return ASDF_EINVAL;
  const int chunks = chunks_of(num_faces);
  const size_t can_split = split_bytes(num_faces, M);
  const int shape = shape_from_env();
  if (shape < 0) return ASDF_EINVAL;
  if (shape == ASDF_MESH_SDF_SHAPE_SPLIT && M > 0 && chunks > 0 && (!can_split || !scratch_dev)) return ASDF_EINVAL;
  if (M == 0 || (!sdf_dev && !winding_dev && !face_dev && !closest_dev)) return ASDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const float4* ws = reinterpret_cast<const float4*>(workspace_dev);
  const bool winding = sdf_dev || winding_dev;
  const Outputs o = {sdf_dev, winding_dev, (int*)face_dev, closest_dev};
  const long long waves = (M + kWave - 1) / kWave;
  // the switch point: a list that leaves SIMDs idle is split over the chunk range as far as the chunks go
  bool split = can_split && scratch_dev && chunks >= 1 &&
               (shape == ASDF_MESH_SDF_SHAPE_SPLIT || (shape == ASDF_MESH_SDF_SHAPE_AUTO && chunks >= 2 && 2 * waves <= kSplitWaves));
  if (split) {
    const SplitPlan plan = split_plan(chunks, waves);
    const int group_chunks = plan.group_chunks, groups = plan.groups;
    float* part_sum = reinterpret_cast<float*>(scratch_dev);
    float* part_d2 = part_sum + (size_t)chunks * (size_t)M;
    int* part_face = reinterpret_cast<int*>(part_d2 + (size_t)groups * (size_t)M);
    const dim3 grid((unsigned)waves, (unsigned)groups);
    if (winding) {
      hipLaunchKernelGGL((mesh_sdf_pair_kernel<true, true>), grid, dim3(kWave), 0, st, ws, (int)num_faces, xyz_dev, (long long)M, chunks,
                         group_chunks, o, part_sum, part_d2, part_face);
      hipLaunchKernelGGL((mesh_sdf_combine_kernel<true>), dim3((unsigned)waves), dim3(kWave), 0, st, ws, xyz_dev, (long long)M, chunks, groups,
                         o, part_sum, part_d2, part_face);
    } else {
      hipLaunchKernelGGL((mesh_sdf_pair_kernel<false, true>), grid, dim3(kWave), 0, st, ws, (int)num_faces, xyz_dev, (long long)M, chunks,
                         group_chunks, o, part_sum, part_d2, part_face);
      hipLaunchKernelGGL((mesh_sdf_combine_kernel<false>), dim3((unsigned)waves), dim3(kWave), 0, st, ws, xyz_dev, (long long)M, chunks,
                         groups, o, part_sum, part_d2, part_face);
    }
  } else {
    for (long long first = 0; first < M; first += kSliceQueries) {
      const long long m = M - first < kSliceQueries ? M - first : kSliceQueries;
      const Outputs os = {sdf_dev ? sdf_dev + first : nullptr, winding_dev ? winding_dev + first : nullptr,
                          face_dev ? (int*)face_dev + first : nullptr, closest_dev ? closest_dev + 3 * first : nullptr};
      const dim3 grid((unsigned)((m + kWave - 1) / kWave));
      if (winding)
        hipLaunchKernelGGL((mesh_sdf_pair_kernel<true, false>), grid, dim3(kWave), 0, st, ws, (int)num_faces, xyz_dev + 3 * first, m, chunks,
                           chunks, os, (float*)nullptr, (float*)nullptr, (int*)nullptr);
      else
        hipLaunchKernelGGL((mesh_sdf_pair_kernel<false, false>), grid, dim3(kWave), 0, st, ws, (int)num_faces, xyz_dev + 3 * first, m, chunks,
                           chunks, os, (float*)nullptr, (float*)nullptr, (int*)nullptr);
    }
  }
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

}  // extern "C"
