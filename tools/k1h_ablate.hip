// Timing-only ablation / schedule sweep for the split-half decoder kernel (results are NOT checked here - parity lives
// in tests/).  Build (per form: -DPLANES=1 [-DGROUPS=2], -DWIDE=1 [-DSTAMP=1], -DASDF16_STAGE_KB=8):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -w -Ialignsdf_amd/csrc [-DPLANES=1 ...] tools/k1h_ablate.hip -o tools/bin/k1h_x
// (-DWIDE=1 with the flags of its unit in alignsdf_amd/build_native.py as well: -mllvm -pragma-unroll-threshold=200000)
// Run:  k1h_x [N] [data]     data = path of a tools/dump_k1h_inputs.py image (the product's real weights + folded
//                            constants), "zero" (all-zero operands: the DVFS upper bound) or "small" (default: small
//                            pseudo-random weights that keep every ablation finite)
// Besides the launch time the tool reports the shader clock the kernel ran at (s_memtime ticks of workgroup 0 / wall).
// Environment: K1H_STATUS=1 passes a status record like the product does (round 5: that is where three 64-lane LDS atomics per tile
// hid - 14 k clocks the tool never saw), K1H_NOBBOX=1 drops the negative-voxel fold.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifndef STAMP
#define STAMP 0         // 1 (with -DWIDE=1) = the diagnostic build: shader-clock stamps of the record classes of the W form's stages
#endif
#ifndef PLANES
#define PLANES 2        // 1 = the one-plane kernel of the box-only coarse sweep
#endif
#ifndef GROUPS
#define GROUPS 1        // 2 = two point groups per wave (one-plane kernel only)
#endif
#ifndef WIDE
#define WIDE 0          // 1 = the W form (16x16x32 MFMAs; timing only here: it is fed the 32x32x16 image - the same values in another order)
#endif
#ifndef ABL_LIST
#if WIDE && STAMP
#define ABL_LIST X(0)
#elif WIDE        // (the W form's record budget: epilogue 4, barrier 16, LDS-DMA 32 and their combinations; 1 = none of the stream)
#define ABL_LIST X(0) X(4) X(16) X(32) X(20) X(36) X(48) X(52) X(1)
#else
#define ABL_LIST X(0) X(32) X(1) X(16) X(4)
#endif
#endif
#if WIDE && STAMP
// Stamps of the W form's stages (sdf_mlp_f16w_kernel.h: StageStamps16w): s_memtime in front of records 0, 1, 8, 9 and behind record 15
// of every stage, so that a stage falls into four segments - record 0, records 1 .. 7 (the deferred epilogue parts of a tile's first
// stage), record 8 (wait + barrier, first LDS-DMA piece), records 9 .. 15 (one LDS-DMA piece each).  Wave 0 of workgroup 0 adds the
// segments' clocks to g_seg[kind][segment] and counts the stages in g_stages[kind].  A stamp waits for its own result (a scalar memory
// read returns out of order: any LDS wait behind it would otherwise become lgkmcnt(0)), which costs every segment the same ~50 clocks.
__device__ unsigned long long g_seg[3][4];
__device__ unsigned g_stages[3];
#define ASDF16_W_STAMPS
namespace asdf {
struct StageStamps16w {
  unsigned long long t[5];
  __device__ __forceinline__ void at(int kb) {
    const int i = kb == 0 ? 0 : kb == 1 ? 1 : kb == 8 ? 2 : kb == 9 ? 3 : kb == 16 ? 4 : -1;
    if (i >= 0) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t[i]) :: "memory");
  }
  __device__ __forceinline__ void flush(int kind) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) atomicAdd(&g_seg[kind][i], t[i + 1] - t[i]);
      atomicAdd(&g_stages[kind], 1u);
    }
  }
};
}  // namespace asdf
#endif
#if WIDE
#include "sdf_mlp_f16w_kernel.h"
#define K1H_BODY(n) sdf_mlp_f16w_body<n, false>(p);
#else
#include "sdf_mlp_f16_kernel.h"
#define K1H_BODY(n) sdf_mlp_f16_body<false, n, 2, PLANES, GROUPS>(p);
#endif
using namespace asdf;
constexpr int kLds = PLANES == 1 ? kLdsBytesF16P1 : kLdsBytesF16;
__device__ unsigned long long g_ticks[2];
#define X(n) __global__ __launch_bounds__(256, 1) void k_abl_##n(const DecodeParams p) { \
    unsigned long long t0 = __builtin_readcyclecounter(); K1H_BODY(n)  \
    if (blockIdx.x == 0 && threadIdx.x == 0) { g_ticks[0] = t0; g_ticks[1] = __builtin_readcyclecounter(); } }
ABL_LIST
#undef X
int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 128;
  const char* data = argc > 2 ? argv[2] : "small";
  const long long P = (long long)N * N * N;
  float *stream, *cst, *o0, *o1;
  std::vector<uint16_t> h((size_t)kStagesAll * kStageFloats * 2);
  std::vector<float> c(kHeads * kCstFloats);
  if (!strcmp(data, "small")) {
    for (size_t i = 0; i < h.size(); ++i) { _Float16 v = (_Float16)((float)((int)((i * 2654435761u) >> 20) % 2001 - 1000) * 2e-5f); h[i] = *(uint16_t*)&v; }
    for (size_t i = 0; i < c.size(); ++i) c[i] = (float)((int)((i * 40503u) >> 4) % 201 - 100) * 1e-3f;
  } else if (!strcmp(data, "zero")) {
    std::fill(h.begin(), h.end(), 0); std::fill(c.begin(), c.end(), 0.0f);
  } else {
    FILE* f = fopen(data, "rb");
    if (!f || fread(h.data(), 2, h.size(), f) != h.size() || fread(c.data(), 4, c.size(), f) != c.size()) { printf("cannot read %s\n", data); return 1; }
    fclose(f);
  }
  (void)hipMalloc(&stream, h.size() * 4); (void)hipMemcpy(stream, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(reinterpret_cast<char*>(stream) + h.size() * 2, h.data(), h.size() * 2, hipMemcpyHostToDevice);      // (where the W form looks for its image)
  (void)hipMalloc(&cst, c.size() * 4); (void)hipMemcpy(cst, c.data(), c.size() * 4, hipMemcpyHostToDevice);
  (void)hipMalloc(&o0, P * 4); (void)hipMalloc(&o1, P * 4);
  int* bbox; (void)hipMalloc(&bbox, 64); (void)hipMemset(bbox, 0, 64);
  // K1H_STATUS=1: the decoder's status record as the product passes it (peak words, range report, clock stamps); K1H_NOBBOX=1: no box fold
  int* status = nullptr;
  if (getenv("K1H_STATUS")) { (void)hipMalloc(&status, 64); (void)hipMemset(status, 0, 64); }
  // one-plane kernels: the fp16 point-feature / bias operands (timing only: small values, T = 1)
  std::vector<uint16_t> a16h((size_t)kHeads * kA16Floats * 2);
  for (size_t i = 0; i < a16h.size(); ++i) { _Float16 v = strcmp(data, "zero") ? (_Float16)((float)((int)((i * 2654435761u) >> 20) % 201 - 100) * 1e-2f) : (_Float16)0.0f; a16h[i] = *(uint16_t*)&v; }
  for (int h = 0; h < kHeads; ++h) { float one = 1.0f; memcpy(&a16h[((size_t)h * kA16Floats + 2 * kA16LayerFloats) * 2], &one, 4); memcpy(&a16h[((size_t)h * kA16Floats + 2 * kA16LayerFloats + 1) * 2], &one, 4); }
  float* a16; (void)hipMalloc(&a16, a16h.size() * 2); (void)hipMemcpy(a16, a16h.data(), a16h.size() * 2, hipMemcpyHostToDevice);
  DecodeParams p{}; p.stream = stream; p.cst = cst; p.sdf0 = o0; p.sdf1 = o1; p.P = P; p.N = N; p.mode = kGridReference;
  p.vs = 2.0f / (N - 1); p.o0 = p.o1 = p.o2 = -1.f; p.num_mlps = 2; p.first_mlp = 0; p.bbox = getenv("K1H_NOBBOX") ? nullptr : bbox; p.a16 = a16; p.status = status;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const double flop = (double)P * 2 * 3145728.0 / (PLANES == 1 ? 3 : 1);
  printf("GROUPS %d  PLANES %d  PREFETCH %d  BARRIER_KB %d  data %s\n", GROUPS, PLANES, S16<PLANES, GROUPS>::kPrefetch, PLANES == 2 ? kBarrierKb : kBarrierKbP1, data);
  // K1H_ROUNDS (default 3) passes over the list, so that the forms are timed interleaved: per form the best launch of every pass
  const int rounds = getenv("K1H_ROUNDS") ? atoi(getenv("K1H_ROUNDS")) : 3;
  for (int round = 0; round < rounds; ++round) {
#define X(n) { (void)hipFuncSetAttribute((const void*)k_abl_##n, hipFuncAttributeMaxDynamicSharedMemorySize, kLds); \
    float best = 1e9; double ghz = 0; for (int it = 0; it < 4; ++it) { (void)hipEventRecord(e0); hipLaunchKernelGGL(k_abl_##n, dim3(256), dim3(256), kLds, 0, p); \
      (void)hipEventRecord(e1); (void)hipEventSynchronize(e1); float ms; (void)hipEventElapsedTime(&ms, e0, e1); \
      unsigned long long t[2]; (void)hipMemcpyFromSymbol(t, HIP_SYMBOL(g_ticks), 16); \
      if (ms < best) { best = ms; ghz = (double)(t[1] - t[0]) / (ms * 1e6); } } \
    printf("pass %d  ABL %2d  N=%d  %.3f ms  %.0f TF/s f16 MFMA (%.1f%% of 2516)  wg0 ticks/wall = %.3f GHz  err=%d\n", round, n, N, best, flop / best / 1e9, flop / best / 1e9 / 25.166, ghz, (int)hipGetLastError()); }
  ABL_LIST
#undef X
  }
#if WIDE && STAMP
  {
    // clocks per record of wave 0 of workgroup 0, over every launch above (stamps included: ~50 clocks per segment)
    unsigned long long seg[3][4]; unsigned stages[3];
    (void)hipMemcpyFromSymbol(seg, HIP_SYMBOL(g_seg), sizeof(seg)); (void)hipMemcpyFromSymbol(stages, HIP_SYMBOL(g_stages), sizeof(stages));
    const char* kind[3] = {"layer 1 / 3 tile, first stage (epilogue parts in records 1 .. 8)", "layer 1 / 3 tile, second stage (no epilogue)",
                           "layer 2 tile (epilogue parts in records 1 .. 8)"};
    const int recs[4] = {1, 7, 1, 7};
    const char* name[4] = {"record 0", "records 1 .. 7", "record 8 (wait, barrier, DMA piece 0)", "records 9 .. 15 (DMA pieces 1 .. 7)"};
    for (int k = 0; k < 3; ++k) {
      printf("%s: %u stages stamped\n", kind[k], stages[k]);
      for (int i = 0; i < 4; ++i) printf("    %-40s %8.1f clocks per record\n", name[i], stages[k] ? (double)seg[k][i] / stages[k] / recs[i] : 0.0);
    }
  }
#endif
  return 0;
}
