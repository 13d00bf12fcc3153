// Hand-object interaction records (include/alignsdf_hip.h: asdf_interaction_lattice, asdf_interaction_points): two bandwidth
// kernels over plain device arrays - no decoder.  Both walk their input in wave-sized chunks with a wave-UNIFORM loop, so every count
// is one ballot and one scalar add per chunk and never leaves the scalar registers; the box and the minimum ride in a few vector
// registers that only a hit touches.  One set of atomics per workgroup; no LDS beyond that reduction, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/alignsdf_hip.h"
#include "common.h"

namespace asdf {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;          // 256 CUs x 8 workgroups: the rest is grid-stride
constexpr int kIntMax = 0x7fffffff;

__device__ __forceinline__ int popc(unsigned long long m) { return __popcll(m); }

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// the order-preserving key of mc33.hip (float_key): unsigned comparison of keys = comparison of floats, -0.0 below +0.0
__device__ __forceinline__ unsigned float_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned key_bits(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

__global__ void overlap_init_kernel(int* rec) {
  const int i = threadIdx.x;
  if (i < ASDF_OVERLAP_WORDS)
    rec[i] = i >= ASDF_OVERLAP_MIN && i < ASDF_OVERLAP_MIN + 3 ? kIntMax : (i >= ASDF_OVERLAP_MAX && i < ASDF_OVERLAP_MAX + 3 ? -1 : 0);
}

// The running state of a wave: four scalar counts and the per-lane box of the both-negative voxels.
struct Overlap {
  int hand = 0, obj = 0, both = 0, nan = 0;
  int lo0 = kIntMax, lo1 = kIntMax, lo2 = kIntMax, hi0 = -1, hi1 = -1, hi2 = -1;

  // one voxel per lane (lanes without one pass +0.0 twice); i = its linear index
  __device__ __forceinline__ void take(float a, float b, unsigned i, unsigned n1, unsigned n2) {
    const bool na = a < 0.0f, nb = b < 0.0f;
    hand += popc(__ballot(na));
    obj += popc(__ballot(nb));
    nan += popc(__ballot(a != a || b != b));
    const unsigned long long m = __ballot(na && nb);
    if (m) {                                // (wave-uniform: no division where the surfaces are apart)
      both += popc(m);
      if (na && nb) {
        const unsigned r = i / n2, i2 = i - r * n2, i0 = r / n1, i1 = r - i0 * n1;
        lo0 = min(lo0, (int)i0); hi0 = max(hi0, (int)i0);
        lo1 = min(lo1, (int)i1); hi1 = max(hi1, (int)i1);
        lo2 = min(lo2, (int)i2); hi2 = max(hi2, (int)i2);
      }
    }
  }
};

// One streaming pass over two [n0][n1][n2] volumes as flat arrays of n = n0 n1 n2 <= 2^30 floats: `head` (0..3) leading floats up to
// the first 16-byte boundary of `a`, nvec float4 of the aligned body, the rest as the tail.  b_aligned: b + head is 16-byte aligned as
// well (the volumes sit alike in memory) - else its four floats are loaded one by one.
__global__ __launch_bounds__(kThreads) void interaction_lattice_kernel(const float* __restrict__ a, const float* __restrict__ b, unsigned n,
                                                                       unsigned n1, unsigned n2, unsigned head, unsigned nvec, int b_aligned,
                                                                       int* rec) {
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned wave0 = blockIdx.x * kWaves + w, nwaves = gridDim.x * kWaves;
  const unsigned nchunks = (nvec + 63) >> 6;
  Overlap o;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  auto load = [&](const float* p, unsigned i, bool vec) {
    return vec ? *reinterpret_cast<const float4*>(p + i) : make_float4(p[i], p[i + 1], p[i + 2], p[i + 3]);
  };
  // two chunks per trip, all four loads issued before the first value is looked at: a wave keeps 2 x 2 KiB in flight, and the
  // chip enough to cover the HBM latency at its streaming rate (one chunk per trip read at about half of it)
  for (unsigned c = wave0; c < nchunks; c += 2 * nwaves) {
    const unsigned v0 = (c << 6) + lane, v1 = ((c + nwaves) << 6) + lane;      // (v1 >= nvec when the second chunk does not exist)
    const unsigned i0 = head + 4 * v0, i1 = head + 4 * v1;
    float4 qa0 = zero, qb0 = zero, qa1 = zero, qb1 = zero;
    if (v0 < nvec) { qa0 = load(a, i0, true); qb0 = load(b, i0, b_aligned); }
    if (v1 < nvec) { qa1 = load(a, i1, true); qb1 = load(b, i1, b_aligned); }
    o.take(qa0.x, qb0.x, i0, n1, n2);
    o.take(qa0.y, qb0.y, i0 + 1, n1, n2);
    o.take(qa0.z, qb0.z, i0 + 2, n1, n2);
    o.take(qa0.w, qb0.w, i0 + 3, n1, n2);
    o.take(qa1.x, qb1.x, i1, n1, n2);
    o.take(qa1.y, qb1.y, i1 + 1, n1, n2);
    o.take(qa1.z, qb1.z, i1 + 2, n1, n2);
    o.take(qa1.w, qb1.w, i1 + 3, n1, n2);
  }
  if (wave0 == 0) {
    // head and tail, at most three floats each: lanes 0..2 the head, lanes 4..6 the tail
    const unsigned tail0 = head + 4 * nvec;
    unsigned i = n;
    if (lane < head) i = lane;
    else if (lane >= 4 && lane < 8 && tail0 + (lane - 4) < n) i = tail0 + (lane - 4);
    float fa = 0.0f, fb = 0.0f;
    if (i < n) { fa = a[i]; fb = b[i]; }
    o.take(fa, fb, i, n1, n2);
  }
  o.lo0 = wave_min_i32(o.lo0); o.lo1 = wave_min_i32(o.lo1); o.lo2 = wave_min_i32(o.lo2);
  o.hi0 = wave_max_i32(o.hi0); o.hi1 = wave_max_i32(o.hi1); o.hi2 = wave_max_i32(o.hi2);
  // one set of atomics per workgroup, as neg_bbox_kernel
  __shared__ int s_rec[kWaves][10];
  if (lane == 0) {
    int* s = s_rec[w];
    s[0] = o.hand; s[1] = o.obj; s[2] = o.both; s[3] = o.nan;
    s[4] = o.lo0; s[5] = o.lo1; s[6] = o.lo2; s[7] = o.hi0; s[8] = o.hi1; s[9] = o.hi2;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int j = threadIdx.x;
    int v = s_rec[0][j];
    for (int k = 1; k < kWaves; ++k) v = j < 4 ? v + s_rec[k][j] : (j < 7 ? min(v, s_rec[k][j]) : max(v, s_rec[k][j]));
    // (a workgroup without a both-negative voxel holds INT_MAX / -1 here: it leaves the box alone)
    if (j < 4) { if (v) atomicAdd(rec + ASDF_OVERLAP_HAND + j, v); }
    else if (j < 7) { if (v != kIntMax) atomicMin(rec + ASDF_OVERLAP_MIN + (j - 4), v); }
    else if (v != -1) atomicMax(rec + ASDF_OVERLAP_MAX + (j - 7), v);
  }
}

// ---- the value list

constexpr unsigned long long kNoMin = ~0ull;          // no value yet: above every (key, index) pair

// words [6..7] carry the packed (key << 32 | index) minimum between the init and the finish kernel
__global__ void contact_init_kernel(int* rec) {
  const int i = threadIdx.x;
  if (i < ASDF_CONTACT_WORDS) rec[i] = i >= ASDF_CONTACT_WORDS - 2 ? -1 : 0;
}

__global__ void contact_finish_kernel(int* rec) {
  if (threadIdx.x != 0) return;
  const unsigned idx = (unsigned)rec[ASDF_CONTACT_WORDS - 2], key = (unsigned)rec[ASDF_CONTACT_WORDS - 1];
  const bool none = idx == 0xffffffffu && key == 0xffffffffu;
  rec[ASDF_CONTACT_MIN_BITS] = none ? 0x7f800000 : (int)key_bits(key);
  rec[ASDF_CONTACT_ARGMIN] = none ? -1 : (int)idx;
  rec[ASDF_CONTACT_WORDS - 2] = 0;
  rec[ASDF_CONTACT_WORDS - 1] = 0;
}

static_assert(ASDF_CONTACT_WORDS == 8, "the packed minimum sits in words 6 and 7: 8-byte aligned when the record is");

__global__ __launch_bounds__(kThreads) void interaction_points_kernel(const float* __restrict__ f, int cap, const int* __restrict__ count,
                                                                      float tau, int* rec) {
  const unsigned n = count ? (unsigned)min(max(*count, 0), cap) : (unsigned)cap;
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned wave0 = blockIdx.x * kWaves + w, nwaves = gridDim.x * kWaves;
  const unsigned nchunks = (n + 63) >> 6;
  int seen = 0, neg = 0, near = 0, nan = 0;
  unsigned long long best = kNoMin;
  for (unsigned c = wave0; c < nchunks; c += nwaves) {
    const unsigned i = (c << 6) + lane;
    const bool in = i < n;
    const float v = in ? f[i] : 0.0f;
    seen += popc(__ballot(in));
    neg += popc(__ballot(in && v < 0.0f));
    near += popc(__ballot(in && v <= tau));
    nan += popc(__ballot(in && v != v));
    if (in && v == v) {
      const unsigned long long p = ((unsigned long long)float_key(v) << 32) | i;
      best = p < best ? p : best;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, m), hi = __shfl_xor((unsigned)(best >> 32), m);
    const unsigned long long p = ((unsigned long long)hi << 32) | lo;
    best = p < best ? p : best;
  }
  __shared__ int s_cnt[kWaves][4];
  __shared__ unsigned long long s_best[kWaves];
  if (lane == 0) { s_cnt[w][0] = seen; s_cnt[w][1] = neg; s_cnt[w][2] = near; s_cnt[w][3] = nan; s_best[w] = best; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    int v = 0;
    for (int k = 0; k < kWaves; ++k) v += s_cnt[k][j];
    if (v) atomicAdd(rec + ASDF_CONTACT_COUNT + j, v);
  } else if (threadIdx.x == 4) {
    for (int k = 1; k < kWaves; ++k) best = s_best[k] < best ? s_best[k] : best;      // (thread 4 is lane 4 of wave 0: best = s_best[0])
    if (best != kNoMin) atomicMin(reinterpret_cast<unsigned long long*>(rec + ASDF_CONTACT_WORDS - 2), best);
  }
}

}  // namespace
}  // namespace asdf

using namespace asdf;

extern "C" {

int asdf_interaction_lattice(const float* vol_hand_dev, const float* vol_obj_dev, int32_t n0, int32_t n1, int32_t n2, int32_t* rec_dev,
                             void* stream) {
  if (!vol_hand_dev || !vol_obj_dev || !rec_dev || n0 < 1 || n1 < 1 || n2 < 1) return ASDF_EINVAL;
  const unsigned long long n = (unsigned long long)n0 * (unsigned long long)n1 * (unsigned long long)n2;
  if (n > (1ull << 30) || (((uintptr_t)vol_hand_dev | (uintptr_t)vol_obj_dev | (uintptr_t)rec_dev) & 3)) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  unsigned head = (unsigned)(((16 - ((uintptr_t)vol_hand_dev & 15)) & 15) >> 2);
  if (head > n) head = (unsigned)n;
  const unsigned nvec = ((unsigned)n - head) >> 2;
  const int b_aligned = (((uintptr_t)(vol_obj_dev + head)) & 15) == 0;
  const unsigned long long chunks = ((unsigned long long)nvec + 63) >> 6;
  const unsigned long long want = (chunks + kWaves - 1) / kWaves;
  const int grid = (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
  hipLaunchKernelGGL(overlap_init_kernel, dim3(1), dim3(64), 0, st, rec_dev);
  hipLaunchKernelGGL(interaction_lattice_kernel, dim3(grid), dim3(kThreads), 0, st, vol_hand_dev, vol_obj_dev, (unsigned)n, (unsigned)n1,
                     (unsigned)n2, head, nvec, b_aligned, rec_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_interaction_points(const float* sdf_dev, int32_t cap, const int32_t* count_dev, float tau, int32_t* rec_dev, void* stream) {
  if (cap < 0 || (!sdf_dev && cap > 0) || !rec_dev || !(tau >= 0.0f)) return ASDF_EINVAL;
  if (((uintptr_t)sdf_dev & 3) || ((uintptr_t)count_dev & 3) || ((uintptr_t)rec_dev & 7)) return ASDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(contact_init_kernel, dim3(1), dim3(64), 0, st, rec_dev);
  if (cap > 0) {
    const long long want = ((long long)cap + kThreads - 1) / kThreads;
    const int grid = (int)(want > kMaxBlocks ? kMaxBlocks : want);
    hipLaunchKernelGGL(interaction_points_kernel, dim3(grid), dim3(kThreads), 0, st, sdf_dev, (int)cap, (const int*)count_dev, tau, rec_dev);
  }
  hipLaunchKernelGGL(contact_finish_kernel, dim3(1), dim3(64), 0, st, rec_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

}  // extern "C"
