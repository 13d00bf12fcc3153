// Bookkeeping kernels of the sweeps (included by decoder.hip): box records, voxel lists, band marks, the audit picks, the zoom
// cube and the sweep record.  The records they index are laid out in include/alignsdf_hip.h and sweep_records.h.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_mlp_common.h"

namespace asdf {

__global__ void bbox_init_kernel(int* bbox) {   // both heads empty
  const int i = threadIdx.x;
  if (i < ASDF_BOX_WORDS) bbox[i] = empty_box_word(i & (ASDF_BOX_STRIDE - 1));
}

// Start of a one-plane sweep: the box record plus every small counter / flag word the sweep's kernels accumulate into, in ONE
// launch (they were a bbox_init launch and four memsets: seven launches per sample that the small lattices notice).
struct ClearRange { int* p; int n; };
__global__ void sweep_init_kernel(int* bbox, ClearRange a, ClearRange b, ClearRange c, ClearRange e) {
  const int i = threadIdx.x;
  if (i < ASDF_BOX_WORDS) bbox[i] = empty_box_word(i & (ASDF_BOX_STRIDE - 1));
  if (i < a.n) a.p[i] = 0;
  if (i < b.n) b.p[i] = 0;
  if (i < c.n) c.p[i] = 0;
  if (i < e.n) e.p[i] = 0;
}

// K2 (standalone form; K1 fuses the same reduction into its epilogue): bounding box of the voxels with
// sdf < 0 - torch.nonzero + per-axis min/max of get_higher_res_cube (utils/mesh.py:208-237).
// One wave per (i0, i1) row: the row index is wave-uniform (no per-voxel division), lanes stride over axis 2 with float4
// loads when the row length allows; HBM-bound streaming read (4 n bytes).  `flag`: when non-null the kernel is a no-op
// unless *flag != 0 (the conditional recount behind the near-level refinement).
__global__ __launch_bounds__(256) void neg_bbox_kernel(const float* __restrict__ vol, int n0, int n1, int n2, int* bbox, const int* flag) {
  if (flag && *flag == 0) return;
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)n0 * n1;
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  int lo0 = 0x7fffffff, lo1 = 0x7fffffff, lo2 = 0x7fffffff, hi0 = -1, hi1 = -1, hi2 = -1, cnt = 0;
  const bool vec = (n2 & 3) == 0 && ((size_t)vol & 15) == 0;
  for (long long r = wave0; r < rows; r += nwaves) {
    const float* row = vol + r * n2;
    int rlo = 0x7fffffff, rhi = -1, rc = 0;
    if (vec) {
      for (int x = lane * 4; x < n2; x += 256) {
        const float4 q = *reinterpret_cast<const float4*>(row + x);
        if (q.x < 0.0f) { rlo = min(rlo, x); rhi = max(rhi, x); ++rc; }
        if (q.y < 0.0f) { rlo = min(rlo, x + 1); rhi = max(rhi, x + 1); ++rc; }
        if (q.z < 0.0f) { rlo = min(rlo, x + 2); rhi = max(rhi, x + 2); ++rc; }
        if (q.w < 0.0f) { rlo = min(rlo, x + 3); rhi = max(rhi, x + 3); ++rc; }
      }
    } else {
      for (int x = lane; x < n2; x += 64)
        if (row[x] < 0.0f) { rlo = min(rlo, x); rhi = max(rhi, x); ++rc; }
    }
    if (rc) {
      const int i0 = (int)(r / n1), i1 = (int)(r % n1);
      lo0 = min(lo0, i0); hi0 = max(hi0, i0); lo1 = min(lo1, i1); hi1 = max(hi1, i1);
      lo2 = min(lo2, rlo); hi2 = max(hi2, rhi); cnt += rc;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo0 = min(lo0, __shfl_xor(lo0, m)); lo1 = min(lo1, __shfl_xor(lo1, m)); lo2 = min(lo2, __shfl_xor(lo2, m));
    hi0 = max(hi0, __shfl_xor(hi0, m)); hi1 = max(hi1, __shfl_xor(hi1, m)); hi2 = max(hi2, __shfl_xor(hi2, m));
    cnt += __shfl_xor(cnt, m);
  }
  // one set of atomics per WORKGROUP (a set per wave on seven hot words serialised 16 k waves: 0.8 ms)
  __shared__ int s_rec[4][7];
  const int w = threadIdx.x >> 6;
  if (lane == 0) { s_rec[w][0] = lo0; s_rec[w][1] = lo1; s_rec[w][2] = lo2; s_rec[w][3] = hi0; s_rec[w][4] = hi1; s_rec[w][5] = hi2; s_rec[w][6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      lo0 = min(lo0, s_rec[k][0]); lo1 = min(lo1, s_rec[k][1]); lo2 = min(lo2, s_rec[k][2]);
      hi0 = max(hi0, s_rec[k][3]); hi1 = max(hi1, s_rec[k][4]); hi2 = max(hi2, s_rec[k][5]); cnt += s_rec[k][6];
    }
    if (cnt) flush_box(bbox, lo0, lo1, lo2, hi0, hi1, hi2, cnt);
  }
}

// Voxels whose value lies within tau of the iso level, of one or two volumes swept on the same lattice: their linear
// indices are appended to idx (order arbitrary), *count counts all of them (also those beyond cap: ASDF_STATUS_LIST_OVERFLOW then counts
// the voxels that could not be listed).  float4 path when n is a multiple of 4.
__global__ __launch_bounds__(256) void collect_near_level_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                                 float tau, int* idx, int* count, int cap, int* status) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  auto hit = [&](long long i) {
    const int k = atomicAdd(count, 1);
    if (k < cap) idx[k] = (int)i;
    else if (status) atomicAdd(status + ASDF_STATUS_LIST_OVERFLOW, 1);
  };
  if ((n & 3) == 0) {
    for (long long q = t0; q < n / 4; q += stride) {
      float4 va = a ? reinterpret_cast<const float4*>(a)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
      float4 vb = b ? reinterpret_cast<const float4*>(b)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
      if (fabsf(va.x) < tau || fabsf(vb.x) < tau) hit(4 * q + 0);
      if (fabsf(va.y) < tau || fabsf(vb.y) < tau) hit(4 * q + 1);
      if (fabsf(va.z) < tau || fabsf(vb.z) < tau) hit(4 * q + 2);
      if (fabsf(va.w) < tau || fabsf(vb.w) < tau) hit(4 * q + 3);
    }
  } else {
    for (long long i = t0; i < n; i += stride)
      if ((a && fabsf(a[i]) < tau) || (b && fabsf(b[i]) < tau)) hit(i);
  }
}

// The candidates of the box-only sweep: voxels whose one-plane value v is not decided by the error bound (-tau <= v < tau)
// for a head, and which lie outside that head's box of certainly negative voxels (v < -tau) - only those can move the box.
// Both heads of a listed voxel are re-evaluated exactly.
__global__ __launch_bounds__(256) void collect_box_candidates_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, float tau,
                                                                     const int* __restrict__ bbox, int* idx, int* count, int cap, int* status) {
  const long long n = (long long)N * N * N;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int box[2][7];      // [ASDF_BOX_MIN .. ASDF_BOX_COUNT] of both heads
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int k = 0; k < 7; ++k) box[h][k] = bbox[ASDF_BOX_STRIDE * h + k];
  auto outside = [&](int h, int i0, int i1, int i2) {
    const int* lo = box[h] + ASDF_BOX_MIN, *hi = box[h] + ASDF_BOX_MAX;
    return box[h][ASDF_BOX_COUNT] == 0 || i0 < lo[0] || i0 > hi[0] || i1 < lo[1] || i1 > hi[1] || i2 < lo[2] || i2 > hi[2];
  };
  auto open = [&](float v) { return v >= -tau && v < tau; };
  // The list is gathered per workgroup in LDS and handed over with ONE reservation per 8 steps: a pose-aligned decoder lists up
  // to 1e6 voxels, and one atomic per wave and step on the single count word was 0.3 ms of same-address atomics.
  constexpr int kSteps = 8, kLocal = kSteps * 256 * 4;
  __shared__ int s_list[kLocal];
  __shared__ int s_n, s_base;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  auto append = [&](bool h, long long i) {
    const unsigned long long m = __ballot(h);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&s_n, __popcll(m));
    base = __shfl(base, leader);
    if (h) s_list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)i;      // (at most kLocal voxels between two flushes)
  };
  auto flush = [&]() {
    __syncthreads();
    const int m = s_n;
    if (threadIdx.x == 0 && m > 0) s_base = atomicAdd(count, m);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
      const int k = s_base + j;
      if (k < cap) idx[k] = s_list[j];
      else if (status) atomicAdd(status + ASDF_STATUS_LIST_OVERFLOW, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
  };
  const bool vec = (N & 3) == 0;
  const long long items = vec ? n / 4 : n;
  const long long rounds = (items + stride - 1) / stride;              // (every thread takes every step: appends and flushes are collective)
  for (long long r = 0; r < rounds; ++r) {
    const long long q = t0 + r * stride;
    const bool live = q < items;
    const long long i = vec ? 4 * q : q;
    const int i2 = (int)(i % N), i1 = (int)((i / N) % N), i0 = (int)((i / N) / N);
    float va[4] = {1.f, 1.f, 1.f, 1.f}, vb[4] = {1.f, 1.f, 1.f, 1.f};
    if (live) {
      if (vec) {
        if (a) { const float4 t = reinterpret_cast<const float4*>(a)[q]; va[0] = t.x; va[1] = t.y; va[2] = t.z; va[3] = t.w; }
        if (b) { const float4 t = reinterpret_cast<const float4*>(b)[q]; vb[0] = t.x; vb[1] = t.y; vb[2] = t.z; vb[3] = t.w; }
      } else {
        if (a) va[0] = a[i];
        if (b) vb[0] = b[i];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!vec && k > 0) break;
      append(live && ((a && open(va[k]) && outside(0, i0, i1, i2 + k)) || (b && open(vb[k]) && outside(1, i0, i1, i2 + k))), i + k);
    }
    if ((r + 1) % kSteps == 0) flush();
  }
  flush();
}

// The candidate count decides how the candidates are re-evaluated (the host cannot know it without a wait, so both forms are
// enqueued and the one whose count word is zero returns at once): up to `direct` voxels straight on the fp32 chain - one round of
// 128-point tiles over the CUs is the latency floor of that chain anyway; more than that (pose-aligned decoders list up to 1e6)
// through the split-half kernel first, 3 x the fp32 chain's rate, and the fp32 chain only where those values lie within refine_tau
// of the level - the rule of every split-half sweep.  out[0] / out[1]: the count as the direct / the two-step form sees it,
// out[2] = 0: the near-level count of the two-step form.
__global__ void split_candidate_count_kernel(const int* __restrict__ count, int cap, int direct, int* out) {
  if (threadIdx.x == 0) {
    int c = *count;
    if (c > cap) c = cap;
    out[0] = c <= direct ? c : 0;
    out[1] = c > direct ? c : 0;
    out[2] = 0;
  }
}

// ... and the two-step form's last step: every listed voxel whose exact value is negative extends its head's box (a voxel the
// sweep kernel had counted already changes nothing: min / max; the count words only have to be non-zero iff there is a negative voxel)
__global__ __launch_bounds__(256) void extend_box_from_list_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const int* __restrict__ list, const int* __restrict__ count, int N, int* bbox) {
  const int n = *count;
  const float* vols[2] = {a, b};
  int lo[2][3], hi[2][3], cnt[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[h][k] = 0x7fffffff; hi[h][k] = -1; }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int po = list[i];
    const int i2 = po % N, i1 = (po / N) % N, i0 = (po / N) / N;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (vols[h] && vols[h][po] < 0.0f) {
        lo[h][0] = min(lo[h][0], i0); lo[h][1] = min(lo[h][1], i1); lo[h][2] = min(lo[h][2], i2);
        hi[h][0] = max(hi[h][0], i0); hi[h][1] = max(hi[h][1], i1); hi[h][2] = max(hi[h][2], i2);
        ++cnt[h];
      }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (!vols[h]) continue;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        lo[h][k] = min(lo[h][k], __shfl_xor(lo[h][k], off));
        hi[h][k] = max(hi[h][k], __shfl_xor(hi[h][k], off));
      }
      cnt[h] += __shfl_xor(cnt[h], off);
    }
    if ((threadIdx.x & 63) == 0 && cnt[h] > 0)
      flush_box(bbox + ASDF_BOX_STRIDE * h, lo[h][0], lo[h][1], lo[h][2], hi[h][0], hi[h][1], hi[h][2], cnt[h]);
  }
}

// The narrow-band fine sweep (asdf_decode_grid_band).  Marching cubes reads a cell's eight corner values only if the cell is
// active, and otherwise only their signs.  With one-plane values v known to lie within tau of the exact ones, a cell CAN be
// active only if its corners' one-plane signs are mixed or one of them is undecided (|v| < tau): for those cells all eight
// corners are marked for exact re-evaluation; every other cell is inactive whatever the error, and its corners are never read.
// One thread per 4 x-consecutive cells, like mc_classify: 4 corner rows of 5 values.
// (round 5: z from blockIdx.y, (y, group) from a 32-bit index - no 64-bit divisions - and the four corner rows as one 16-byte load
// plus one word each where the row length allows: 80 -> about 30 us per 256^3 volume; same marks)
__global__ __launch_bounds__(256) void band_mark_kernel(const float* __restrict__ vol, int N, float tau, unsigned char* __restrict__ mark) {
  const int cx = N - 1, groups = (cx + 3) >> 2;
  const int per_slab = groups * cx;                   // (y, group) pairs of one z
  const bool vec = (N & 3) == 0;                      // rows start 16-byte aligned and x0 is a multiple of 4
  for (int z = blockIdx.y; z < cx; z += gridDim.y) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < per_slab; g += gridDim.x * blockDim.x) {
      const int y = g / groups, x0 = (g - y * groups) * 4;
      const float* r00 = vol + ((size_t)z * N + y) * N;
      const float* rows[4] = {r00, r00 + N, r00 + (size_t)N * N, r00 + (size_t)N * N + N};
      unsigned pos[4], neg[4];           // bit i: value i of the row is certainly positive / certainly negative
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[5];
        if (vec) {
          const float4 t = *reinterpret_cast<const float4*>(rows[q] + x0);
          v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
          v[4] = x0 + 4 < N ? rows[q][x0 + 4] : 0.0f;
        } else {
#pragma unroll
          for (int i = 0; i < 5; ++i) v[i] = x0 + i < N ? rows[q][x0 + i] : 0.0f;
        }
        pos[q] = neg[q] = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          if (x0 + i < N) {
            pos[q] |= (v[i] >= tau ? 1u : 0u) << i;
            neg[q] |= (v[i] < -tau ? 1u : 0u) << i;
          } else {
            pos[q] |= 1u << i; neg[q] |= 1u << i;      // beyond the row: neutral for the AND reductions below, cells there are masked off
          }
        }
      }
      // a cell is certainly inactive iff all 8 corners are certainly positive, or all certainly negative
      const unsigned ap = pos[0] & pos[1] & pos[2] & pos[3], an = neg[0] & neg[1] & neg[2] & neg[3];
      const int ncell = min(4, cx - x0);
      const unsigned inactive = (ap & (ap >> 1)) | (an & (an >> 1));
      const unsigned cand = ~inactive & ((1u << ncell) - 1);
      if (!cand) continue;
      // corners of the candidate cells: columns x0 + i and x0 + i + 1 of the four rows
      const unsigned cols = (cand | (cand << 1)) & 0x1fu;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned char* m = mark + (rows[q] - vol);
#pragma unroll
        for (int i = 0; i < 5; ++i)
          if ((cols >> i) & 1) m[x0 + i] = 1;
      }
    }
  }
}

// marked voxels -> index list (order arbitrary); *count counts all of them, also those beyond cap.  One reservation on the count
// word per WORKGROUP and round (wave scans + an LDS hand-over): half a million marked voxels used to be ~1e5 same-address atomics.
// `done` / `count_copy` (optional): the last workgroup to finish copies the final count to *count_copy - the first audit position of the
// list (the audit picks are appended behind the marked voxels); *done must be zero at launch (sweep_init_kernel).  Was a separate
// 4-byte device-to-device copy per head.
__global__ __launch_bounds__(256) void band_compact_kernel(const unsigned char* __restrict__ mark, long long n, int* idx, int* count, int cap,
                                                           int* done, int* count_copy) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long items = (n + 15) / 16;
  const long long rounds = (items + stride - 1) / stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int s_wave[4], s_base;
  for (long long r = 0; r < rounds; ++r) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x + r * stride;
    unsigned ww[4] = {0u, 0u, 0u, 0u};
    if (q < items) {
      if (q * 16 + 16 <= n) {
        const uint4 w = reinterpret_cast<const uint4*>(mark)[q];
        ww[0] = w.x; ww[1] = w.y; ww[2] = w.z; ww[3] = w.w;
      } else {
        for (long long i = q * 16; i < n; ++i)
          if (mark[i]) ww[(i - q * 16) >> 2] |= 1u << (8 * ((i - q * 16) & 3));
      }
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += __popc(ww[k] & 0x01010101u);
    // exclusive position of this thread's entries inside the workgroup's reservation
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
      s_base = total ? atomicAdd(count, total) : 0;
    }
    __syncthreads();
    int at = s_base + (incl - c);
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    if (c) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if ((ww[k] >> (8 * b)) & 1) { if (at < cap) idx[at] = (int)(q * 16 + 4 * k + b); ++at; }
    }
    __syncthreads();
  }
  // (no fence: thread 0 issued this workgroup's reservations on *count itself and has their return values - they are complete -
  // before it arrives here, and device-scope atomics are coherent across the XCDs.  A __threadfence() per workgroup is an L2
  // write-back each: 19 -> 131 us per launch at N = 256, seen in the kernel statistics)
  if (done && threadIdx.x == 0 && atomicAdd(done, 1) == (int)gridDim.x - 1) *count_copy = atomicAdd(count, 0);
}

// near-level voxels among the LISTED ones of one volume (the narrow-band sweep refines only where it re-evaluated)
__global__ __launch_bounds__(256) void collect_near_level_list_kernel(const float* __restrict__ vol, const int* __restrict__ list,
                                                                      const int* __restrict__ list_count, int list_cap, float tau, int* idx,
                                                                      int* count, int cap, int* status) {
  const int n = *list_count < list_cap ? *list_count : list_cap;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int v = list[i];
    if (fabsf(vol[v]) < tau) {
      const int k = atomicAdd(count, 1);
      if (k < cap) idx[k] = v;
      else if (status) atomicAdd(status + ASDF_STATUS_LIST_OVERFLOW, 1);
    }
  }
}

// The audit of a one-plane sweep: n voxels drawn uniformly at random (splitmix64 of seed + k, with replacement) from those the
// sweep DECIDED BY SIGN ALONE - not marked for re-evaluation (band sweep: mark[v] == 0, which implies |value| >= tau), or
// outside [-tau, tau) for every evaluated head (box sweep) - are appended to a voxel list; the caller re-evaluates them with
// the split-half kernel, which reports the largest |exact - one-plane| over them and the number whose sign was wrong.
// One reservation per wave.
__device__ __forceinline__ unsigned long long splitmix64_dev(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The AT-RISK SHELL of a one-plane sweep (round 4): of the voxels a sweep decides by sign alone, only those whose one-plane value
// lies close to the decision threshold can be decided wrongly by an error of the allowance's order - tau <= |v| < 2 tau.  A uniform
// draw spends a fraction of a percent of its picks there; half of the audit is therefore drawn FROM the shell: it is counted
// (shell_count_kernel) and then listed - every shell voxel while the shell is smaller than the budget (an exhaustive check), a
// hash-thinned uniform subset of expected size `budget` otherwise (shell_pick_kernel).  Band sweep: unmarked voxels of one head's
// volume (unmarked implies |v| >= tau); box sweep: voxels every evaluated head leaves outside [-tau, tau), some head inside 2 tau.
__device__ __forceinline__ bool in_audit_shell(const float* __restrict__ a, const float* __restrict__ b,
                                               const unsigned char* __restrict__ mark, long long v, float tau) {
  if (mark) return mark[v] == 0 && (fabsf(a[v]) < 2.0f * tau || (b && fabsf(b[v]) < 2.0f * tau));      // (b: a CombinedDecoder's second column)
  bool decided = true, close = false;
  if (a) { const float t = a[v]; decided = decided && !(t >= -tau && t < tau); close = close || fabsf(t) < 2.0f * tau; }
  if (b) { const float t = b[v]; decided = decided && !(t >= -tau && t < tau); close = close || fabsf(t) < 2.0f * tau; }
  return decided && close;
}
__device__ __forceinline__ void audit_pick_block(int k, const float* __restrict__ a, const float* __restrict__ b, const unsigned char* __restrict__ mark,
                                                 long long P, float tau, unsigned long long seed, int n, int* list, int* count, int cap) {
  bool ok = k < n;
  long long v = 0;
  if (ok) {
    v = (long long)(splitmix64_dev(seed + (unsigned long long)k * 0xD1342543DE82EF95ull) % (unsigned long long)P);
    if (mark) ok = mark[v] == 0;
    else {
      if (a) { const float t = a[v]; ok = ok && !(t >= -tau && t < tau); }
      if (b) { const float t = b[v]; ok = ok && !(t >= -tau && t < tau); }
    }
  }
  const unsigned long long m = __ballot(ok);
  if (!m) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(m));
  base = __shfl(base, 0);
  const int at = base + __popcll(m & ((1ull << lane) - 1));
  if (ok && at < cap) list[at] = (int)v;
}
__global__ __launch_bounds__(256) void audit_pick_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const unsigned char* __restrict__ mark, long long P, float tau,
                                                         unsigned long long seed, int n, int* list, int* count, int cap) {
  audit_pick_block(blockIdx.x * blockDim.x + threadIdx.x, a, b, mark, P, tau, seed, n, list, count, cap);
}
// workgroups 0 .. shell_blocks - 1 count the shell; the ones behind them draw the `uniform_n` uniform picks (audit_pick_kernel's draw:
// the two were separate launches - the small lattices notice every launch)
__global__ __launch_bounds__(256) void shell_count_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const unsigned char* __restrict__ mark, long long P, float tau, int* shell_n,
                                                          int shell_blocks, unsigned long long seed, int uniform_n, int* list, int* count, int cap) {
  if ((int)blockIdx.x >= shell_blocks) {
    audit_pick_block(((int)blockIdx.x - shell_blocks) * blockDim.x + threadIdx.x, a, b, mark, P, tau, seed, uniform_n, list, count, cap);
    return;
  }
  const long long stride = (long long)shell_blocks * blockDim.x;
  int c = 0;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < P; v += stride) c += in_audit_shell(a, b, mark, v, tau) ? 1 : 0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  __shared__ int s_c[4];
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) { const int t = s_c[0] + s_c[1] + s_c[2] + s_c[3]; if (t) atomicAdd(shell_n, t); }
}
__global__ __launch_bounds__(256) void shell_pick_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const unsigned char* __restrict__ mark, long long P, float tau,
                                                         unsigned long long seed, int budget, const int* __restrict__ shell_n,
                                                         int* list, int* count, int cap, int* audit_rec) {
  const int population = *shell_n;
  // keep every shell voxel while they fit the budget, else each with probability budget / population (a hash of the voxel index)
  const unsigned long long thr = population <= budget ? (1ull << 32) : (unsigned long long)(((double)budget / (double)population) * 4294967296.0);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const long long rounds = (P + stride - 1) / stride;
  // the picks of a workgroup are gathered in LDS and handed over with ONE reservation on the list's count word (32 k picks were
  // 32 k same-address atomics: 0.19 ms per launch); what does not fit the LDS list goes straight to the global one
  constexpr int kLocal = 2048;
  __shared__ int s_list[kLocal];
  __shared__ int s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int kept = 0;
  for (long long r = 0; r < rounds; ++r) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x + r * stride;
    const bool ok = v < P && in_audit_shell(a, b, mark, v, tau) &&
                    (splitmix64_dev(seed ^ ((unsigned long long)v * 0x9E3779B97F4A7C15ull)) >> 32) < thr;
    const unsigned long long m = __ballot(ok);
    if (!m) continue;
    int base = 0;
    if (lane == 0) base = atomicAdd(&s_n, __popcll(m));
    base = __shfl(base, 0);
    const int at = base + __popcll(m & ((1ull << lane) - 1));
    if (ok) {
      if (at < kLocal) s_list[at] = (int)v;
      else { const int k = atomicAdd(count, 1); if (k < cap) { list[k] = (int)v; ++kept; } }
    }
  }
  __syncthreads();
  const int nl = s_n < kLocal ? s_n : kLocal;
  if (threadIdx.x == 0) s_base = nl ? atomicAdd(count, nl) : 0;
  __syncthreads();
  for (int j = threadIdx.x; j < nl; j += blockDim.x) {
    const int k = s_base + j;
    if (k < cap) { list[k] = s_list[j]; ++kept; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) kept += __shfl_xor(kept, m);
  if (lane == 0 && kept) atomicAdd(audit_rec + kAuditShellPicks, kept);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(audit_rec + kAuditShellPop, population);
}

// more voxels lay within the refinement threshold of the level than the list holds (ASDF_STATUS_LIST_OVERFLOW != 0): a flag bit of
// the range word of the bbox record tells the caller, who reads that record anyway
// ... and another that the cluster form of the short-list kernel has reported a member that never arrived (ASDF_STATUS_CLUSTER_FAULT,
// sticky: the list was evaluated by the tile form instead - the result is complete - and the host switches the cluster form off)
__global__ void near_overflow_to_bbox_kernel(const int* status, int* bbox) {
  if (threadIdx.x == 0 && status[ASDF_STATUS_LIST_OVERFLOW] != 0) atomicOr(bbox + ASDF_BOX_RANGE, ASDF_BOX_NEAR_OVERFLOW_BIT);
  if (threadIdx.x == 0 && status[ASDF_STATUS_CLUSTER_FAULT] != 0) atomicOr(bbox + ASDF_BOX_RANGE, ASDF_BOX_CLUSTER_FAULT_BIT);
}

__global__ void bbox_reinit_keep_flags_kernel(int* bbox, const int* flag) {   // the range words (the fp16 range report) survive
  if (flag && *flag == 0) return;
  const int i = threadIdx.x;
  if (i < ASDF_BOX_WORDS && (i & (ASDF_BOX_STRIDE - 1)) != ASDF_BOX_RANGE) bbox[i] = empty_box_word(i & (ASDF_BOX_STRIDE - 1));
}

// get_higher_res_cube's arithmetic (utils/mesh.py:239-254) on the boxes of a coarse pass' record, in fp32 like the reference's CPU
// tensors: min / max over the enabled branches (an empty branch contributes zeros, :209-211, :225-227), every operation rounded
// separately (the file is built with -ffp-contract=off; the _rn intrinsics say so again).
extern "C" __global__ void zoom_cube_kernel(const int* __restrict__ bbox, int N, float vs, int use_hand, int use_obj, float* __restrict__ lattice) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float lo[3], hi[3];
  bool first = true;
  for (int h = 0; h < 2; ++h) {
    if (!(h == 0 ? use_hand : use_obj)) continue;
    const int* b = bbox + ASDF_BOX_STRIDE * h;
    const bool any = b[ASDF_BOX_COUNT] != 0;
    for (int a = 0; a < 3; ++a) {
      const float l = any ? (float)b[ASDF_BOX_MIN + a] : 0.0f, u = any ? (float)b[ASDF_BOX_MAX + a] : 0.0f;
      lo[a] = first ? l : fminf(lo[a], l);
      hi[a] = first ? u : fmaxf(hi[a], u);
    }
    first = false;
  }
  if (first) { for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.0f; }
  float span = __fsub_rn(hi[0], lo[0]);
  span = fmaxf(span, __fsub_rn(hi[1], lo[1]));
  span = fmaxf(span, __fsub_rn(hi[2], lo[2]));
  const float cube = __fmul_rn(__fadd_rn(span, 4.0f), vs);
  lattice[3] = __fdiv_rn(cube, (float)(N - 1));
  for (int a = 0; a < 3; ++a) lattice[a] = __fsub_rn(__fmul_rn(__fsub_rn(lo[a], 2.0f), vs), 1.0f);
}

// the status copy and the words behind it of the record of a one-plane sweep, gathered on the device behind the call
extern "C" __global__ void sweep_record_kernel(int* rec, const int* status, const int* near_count, const int* audit_rec) {
  const int i = threadIdx.x;
  if (i < ASDF_STATUS_WORDS) rec[ASDF_REC_STATUS + i] = status[i];
  if (i == 0) {
    rec[ASDF_REC_CANDIDATES] = near_count ? *near_count : 0;
    rec[ASDF_REC_BAND] = audit_rec[kAuditFrom];          // band sweep: voxels marked for the hand / object head (0 for the box sweep)
    rec[ASDF_REC_BAND + 1] = audit_rec[kAuditFrom + 1];
    rec[ASDF_REC_AUDIT_MAX_ERR] = audit_rec[kAuditMaxErr]; rec[ASDF_REC_AUDIT_FLIPS] = audit_rec[kAuditFlips]; rec[ASDF_REC_AUDIT_EVALS] = audit_rec[kAuditEvals];
    rec[ASDF_REC_NEAR_OVERFLOW] = status[ASDF_STATUS_LIST_OVERFLOW];
    rec[ASDF_REC_SHELL_PICKS] = audit_rec[kAuditShellPicks];
    rec[ASDF_REC_SHELL_POPULATION] = audit_rec[kAuditShellPop];
    rec[ASDF_REC_AUDIT_SUMSQ] = audit_rec[kAuditSumSq];
    for (int k = ASDF_REC_AUDIT_SUMSQ + 1; k < ASDF_REC_WORDS; ++k) rec[k] = 0;
  }
}

// Debug hook: the coordinates grid_point() produces, so that the in-kernel lattice can be compared bit for bit with the
// reference's (utils/mesh.py:27-40) - the decoder kernels call the very same device function.
extern "C" __global__ void grid_coords_kernel(float* out, long long first, long long count, int N, int mode, float vs, float o0, float o1, float o2) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  float c0, c1, c2;
  grid_point(first + k, N, mode, vs, o0, o1, o2, c0, c1, c2);
  out[k * 3 + 0] = c0; out[k * 3 + 1] = c1; out[k * 3 + 2] = c2;
}

}  // namespace asdf
