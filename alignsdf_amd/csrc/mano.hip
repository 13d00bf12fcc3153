// The MANO hand layer, forward and reverse (include/alignsdf_hip.h words the rule): pose coefficients and shape values in; vertices,
// 21 joints and the 16 joint transforms out; cotangents of those in, d_pose and d_shape out.  Plain fp32, no contraction.
//
// One workgroup of 256 threads per sample, every intermediate in LDS.  The layer is about a million multiply-adds behind a chain of
// short serial steps (Rodrigues, a four-level chain, and their adjoints), so a launch is latency-bound: the phases below are kept few,
// and each is shaped so that its loads coalesce - the forward reads the blend shapes vertex-fastest ([m][k][V], one vertex per thread),
// the reverse's sums over vertices read them in the model's own order ([V][k][m], one OUTPUT per thread, vertices in index order).
// No atomics and no cross-lane reduction: every sum has one owner and a fixed order, so a sample's bits depend on nothing but the
// sample.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/alignsdf_hip.h"
#include "common.h"

namespace asdf {
namespace {

constexpr int kThreads = 256;
constexpr int kJoints = 16;
constexpr int kMaxV = ASDF_MANO_MAX_VERTS;
constexpr int kPoseMap = 135;   // (R - I) of the 15 finger joints
constexpr int kShape = 10;
constexpr int kHand = 45;       // axis-angle values of the 15 finger joints
constexpr int kAdj = kJoints * 12;

// Where the prepared model lies in the workspace, in 4-byte words.
struct Layout {
  size_t vt, sdt, pdt, pd, sd, w, jt, js, mean, comps, tips, words;
};

__host__ __device__ inline Layout layout_of(int V, int nc) {
  Layout L;
  size_t o = 0;
  const size_t v = (size_t)V;
  L.vt = o, o += 3 * v;                   // v_template                      [3][V]
  L.sdt = o, o += kShape * 3 * v;         // shapedirs                       [10][3][V]
  L.pdt = o, o += kPoseMap * 3 * v;       // posedirs                        [135][3][V]
  L.pd = o, o += v * 3 * kPoseMap;        // posedirs, the model's order     [V][3][135]
  L.sd = o, o += v * 3 * kShape;          // shapedirs, the model's order    [V][3][10]
  L.w = o, o += v * kJoints;              // skinning weights                [V][16]
  L.jt = o, o += kJoints * 3;             // J_regressor x v_template        [16][3]
  L.js = o, o += kJoints * 3 * kShape;    // J_regressor x shapedirs         [16][3][10]
  L.mean = o, o += 48;                    // hands_mean                      [45]
  L.comps = o, o += (size_t)nc * kHand;   // PCA rows                        [nc][45]
  L.tips = o, o += 8;                     // tip vertex ids, clamped to V    int[5]
  L.words = (o + 3) & ~(size_t)3;
  return L;
}

// Fills the workspace.  The joint regressor is folded into the template and the shape directions here, once, with fp64 sums: a
// sample's rest joints are then J = jt + js . beta, ten terms instead of 778.
__global__ __launch_bounds__(kThreads) void mano_prepare_kernel(int V, int nc, const float* __restrict__ v_template,
                                                                const float* __restrict__ shapedirs, const float* __restrict__ posedirs,
                                                                const float* __restrict__ regressor, const float* __restrict__ weights,
                                                                const float* __restrict__ hands_mean, const float* __restrict__ comps,
                                                                const int* __restrict__ tips, float* __restrict__ ws) {
  const Layout L = layout_of(V, nc);
  const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t v = (size_t)V;
  for (size_t i = first; i < 3 * v; i += stride) ws[L.vt + (i % 3) * v + i / 3] = v_template[i];
  for (size_t i = first; i < v * 3 * kShape; i += stride) {
    const size_t l = i % kShape, vk = i / kShape;
    ws[L.sdt + (l * 3 + vk % 3) * v + vk / 3] = shapedirs[i];
    ws[L.sd + i] = shapedirs[i];
  }
  for (size_t i = first; i < v * 3 * kPoseMap; i += stride) {
    const size_t m = i % kPoseMap, vk = i / kPoseMap;
    ws[L.pdt + (m * 3 + vk % 3) * v + vk / 3] = posedirs[i];
    ws[L.pd + i] = posedirs[i];
  }
  for (size_t i = first; i < v * kJoints; i += stride) ws[L.w + i] = weights[i];
  for (size_t i = first; i < kJoints * 3 * (kShape + 1); i += stride) {
    const size_t l = i % (kShape + 1), jk = i / (kShape + 1), j = jk / 3, k = jk % 3;
    double acc = 0.0;
    for (size_t u = 0; u < v; ++u)
      acc += (double)regressor[j * v + u] * (double)(l < kShape ? shapedirs[(u * 3 + k) * kShape + l] : v_template[u * 3 + k]);
    if (l < kShape) ws[L.js + jk * kShape + l] = (float)acc;
    else ws[L.jt + jk] = (float)acc;
  }
  for (size_t i = first; i < 48; i += stride) ws[L.mean + i] = i < kHand ? hands_mean[i] : 0.0f;
  for (size_t i = first; i < (size_t)nc * kHand; i += stride) ws[L.comps + i] = comps[i];
  for (size_t i = first; i < 8; i += stride) {
    int t = i < 5 ? tips[i] : 0;
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);          // (an id outside the model is clamped: no launch reads out of bounds)
    reinterpret_cast<int*>(ws)[L.tips + i] = t;
  }
  for (size_t i = first + L.tips + 8; i < L.words; i += stride) ws[i] = 0.0f;
}

// What both kernels keep of a sample's skeleton.
struct Skeleton {
  float full[48];          // axis-angle values of the 16 joints
  float R[kJoints][9];     // their rotations
  float J[kJoints][3];     // rest joints
  float G[kJoints][12];    // chain transforms, rows of [R | t]
  float A[kJoints][12];    // the same with the rest joint taken out: what skinning blends
};

__device__ inline int parent_of(int j) { return j == 0 ? -1 : ((j - 1) % 3 == 0 ? 0 : j - 1); }

// axis-angle -> rotation by the quaternion route; norm of (a + 1e-8), the quaternion normalised once more
__device__ inline void rodrigues(const float* a, float* R) {
  const float b0 = a[0] + 1e-8f, b1 = a[1] + 1e-8f, b2 = a[2] + 1e-8f;
  const float n = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
  const float h = n * 0.5f, c = cosf(h), s = sinf(h);
  const float q1 = s * (a[0] / n), q2 = s * (a[1] / n), q3 = s * (a[2] / n);
  const float m = sqrtf(((c * c + q1 * q1) + q2 * q2) + q3 * q3);
  const float w = c / m, x = q1 / m, y = q2 / m, z = q3 / m;
  const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  R[0] = ((w2 + x2) - y2) - z2, R[1] = 2.0f * xy - 2.0f * wz, R[2] = 2.0f * wy + 2.0f * xz;
  R[3] = 2.0f * wz + 2.0f * xy, R[4] = ((w2 - x2) + y2) - z2, R[5] = 2.0f * yz - 2.0f * wx;
  R[6] = 2.0f * xz - 2.0f * wy, R[7] = 2.0f * wx + 2.0f * yz, R[8] = ((w2 - x2) - y2) + z2;
}

// the adjoint of exactly the formula above: dR [9] -> da [3]
__device__ inline void rodrigues_adjoint(const float* a, const float* d, float* da) {
  const float b0 = a[0] + 1e-8f, b1 = a[1] + 1e-8f, b2 = a[2] + 1e-8f;
  const float n = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
  const float h = n * 0.5f, c = cosf(h), s = sinf(h);
  const float u0 = a[0] / n, u1 = a[1] / n, u2 = a[2] / n;
  const float q1 = s * u0, q2 = s * u1, q3 = s * u2;
  const float m = sqrtf(((c * c + q1 * q1) + q2 * q2) + q3 * q3);
  const float w = c / m, x = q1 / m, y = q2 / m, z = q3 / m;
  // matrix -> unit quaternion
  const float gw = 2.0f * (w * ((d[0] + d[4]) + d[8]) + ((z * (d[3] - d[1]) + y * (d[2] - d[6])) + x * (d[7] - d[5])));
  const float gx = 2.0f * (x * ((d[0] - d[4]) - d[8]) + ((y * (d[1] + d[3]) + z * (d[2] + d[6])) + w * (d[7] - d[5])));
  const float gy = 2.0f * (y * ((d[4] - d[0]) - d[8]) + ((x * (d[1] + d[3]) + z * (d[5] + d[7])) + w * (d[2] - d[6])));
  const float gz = 2.0f * (z * ((d[8] - d[0]) - d[4]) + ((x * (d[2] + d[6]) + y * (d[5] + d[7])) + w * (d[3] - d[1])));
  // unit quaternion -> quaternion
  const float dot = ((w * gw + x * gx) + y * gy) + z * gz;
  const float gc = (gw - w * dot) / m, g1 = (gx - x * dot) / m, g2 = (gy - y * dot) / m, g3 = (gz - z * dot) / m;
  // quaternion -> (cos, sin, axis); axis = a / n
  const float gs = (g1 * u0 + g2 * u1) + g3 * u2;
  const float gu0 = s * g1, gu1 = s * g2, gu2 = s * g3;
  const float gh = c * gs - s * gc;
  const float gn = 0.5f * gh - (((gu0 * a[0] + gu1 * a[1]) + gu2 * a[2]) / n) / n;
  da[0] = gu0 / n + gn * (b0 / n);
  da[1] = gu1 / n + gn * (b1 / n);
  da[2] = gu2 / n + gn * (b2 / n);
}

// A long sum with one owner: kLanes partial sums over the terms i = lane, lane + kLanes, ... in index order, then a fixed tree over the
// partials.  The order depends on n alone; the shorter chains round less than one serial chain and leave the loads independent.
template <int kLanes, class Term>
__device__ inline float ordered_sum(int n, Term term) {
  float part[kLanes];
#pragma unroll
  for (int k = 0; k < kLanes; ++k) part[k] = 0.0f;
  int i = 0;
  for (; i + kLanes <= n; i += kLanes) {
#pragma unroll
    for (int k = 0; k < kLanes; ++k) part[k] += term(i + k);
  }
#pragma unroll
  for (int k = 0; k < kLanes; ++k)
    if (i + k < n) part[k] += term(i + k);
#pragma unroll
  for (int w = kLanes / 2; w >= 1; w /= 2) {
#pragma unroll
    for (int k = 0; k < w; ++k) part[k] += part[k + w];
  }
  return part[0];
}

// C = A B for 3 x 3 row-major
__device__ inline void mat3_mul(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// The skeleton of sample `b` into LDS: full pose, rotations, rest joints, the chain and the skinning transforms.  Every thread of the
// workgroup calls it; it ends behind a barrier.
__device__ inline void build_skeleton(Skeleton& S, const float* __restrict__ ws, const Layout& L, int nc, const float* __restrict__ pose,
                                      const float* __restrict__ shape, float* __restrict__ hand_pose_out) {
  const int t = threadIdx.x;
  if (t < 3) S.full[t] = pose[t];
  if (t >= 64 && t < 64 + kHand) {
    const int k = t - 64;
    float acc = 0.0f;
    for (int i = 0; i < nc; ++i) acc += pose[3 + i] * ws[L.comps + (size_t)i * kHand + k];
    if (hand_pose_out) hand_pose_out[k] = acc;
    S.full[3 + k] = ws[L.mean + k] + acc;
  }
  if (t >= 128 && t < 128 + kJoints * 3) {
    const int jk = t - 128;
    float acc = 0.0f;
    for (int l = 0; l < kShape; ++l) acc += ws[L.js + (size_t)jk * kShape + l] * shape[l];
    S.J[jk / 3][jk % 3] = ws[L.jt + jk] + acc;
  }
  __syncthreads();
  if (t < kJoints) {
    float a[3] = {S.full[3 * t], S.full[3 * t + 1], S.full[3 * t + 2]}, R[9];
    rodrigues(a, R);
    for (int i = 0; i < 9; ++i) S.R[t][i] = R[i];
  }
  __syncthreads();
  // the chain: thread f < 5 walks finger f from the root outwards, thread 5 writes the root
  if (t < 6) {
    float GR[9], Gt[3];
    for (int i = 0; i < 9; ++i) GR[i] = S.R[0][i];
    for (int i = 0; i < 3; ++i) Gt[i] = S.J[0][i];
    const int first = t < 5 ? 3 * t + 1 : 0, last = t < 5 ? 3 * t + 3 : 0;
    for (int j = first; j <= last; ++j) {
      if (j > 0) {
        const int p = parent_of(j);
        float Rj[9], NR[9], rel[3], Nt[3];
        for (int i = 0; i < 9; ++i) Rj[i] = S.R[j][i];
        for (int i = 0; i < 3; ++i) rel[i] = S.J[j][i] - S.J[p][i];
        mat3_mul(GR, Rj, NR);
        for (int r = 0; r < 3; ++r) Nt[r] = ((GR[3 * r] * rel[0] + GR[3 * r + 1] * rel[1]) + GR[3 * r + 2] * rel[2]) + Gt[r];
        for (int i = 0; i < 9; ++i) GR[i] = NR[i];
        for (int i = 0; i < 3; ++i) Gt[i] = Nt[i];
      }
      for (int r = 0; r < 3; ++r) {
        const float moved = (GR[3 * r] * S.J[j][0] + GR[3 * r + 1] * S.J[j][1]) + GR[3 * r + 2] * S.J[j][2];
        for (int c = 0; c < 3; ++c) S.G[j][4 * r + c] = S.A[j][4 * r + c] = GR[3 * r + c];
        S.G[j][4 * r + 3] = Gt[r];
        S.A[j][4 * r + 3] = Gt[r] - moved;
      }
    }
  }
  __syncthreads();
}

// v_posed of vertex v: template + shape blend + pose blend on R - I of the finger joints
__device__ inline void rest_vertex(const Skeleton& S, const float* __restrict__ ws, const Layout& L, int V, int v, const float* __restrict__ shape,
                                   float* vp) {
  for (int k = 0; k < 3; ++k) {
    float acc = 0.0f;
    for (int l = 0; l < kShape; ++l) acc += ws[L.sdt + ((size_t)l * 3 + k) * V + v] * shape[l];
    vp[k] = acc + ws[L.vt + (size_t)k * V + v];
  }
  float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  const float* pd = ws + L.pdt + v;
#pragma unroll 9
  for (int m = 0; m < kPoseMap; ++m) {
    const int j = 1 + m / 9, e = m % 9;
    const float pm = S.R[j][e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
    b0 += pd[((size_t)m * 3 + 0) * V] * pm;
    b1 += pd[((size_t)m * 3 + 1) * V] * pm;
    b2 += pd[((size_t)m * 3 + 2) * V] * pm;
  }
  vp[0] += b0, vp[1] += b1, vp[2] += b2;
}

// the blended transform of vertex v: rows of [R | t]
__device__ inline void blend_vertex(const Skeleton& S, const float* __restrict__ ws, const Layout& L, int v, float* T) {
  for (int i = 0; i < 12; ++i) T[i] = 0.0f;
  for (int j = 0; j < kJoints; ++j) {
    const float w = ws[L.w + (size_t)v * kJoints + j];
    for (int i = 0; i < 12; ++i) T[i] += S.A[j][i] * w;
  }
}

__device__ inline int joint_source(int i) {          // output joint i <- entry of [16 chain joints, 5 tips]
  constexpr int order[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
  return order[i];
}

__global__ __launch_bounds__(kThreads) void mano_forward_kernel(const float* __restrict__ ws, int V, int nc, const float* __restrict__ pose,
                                                                const float* __restrict__ shape, const float* __restrict__ trans,
                                                                int center_idx, float* __restrict__ verts, float* __restrict__ joints,
                                                                float* __restrict__ global_trans, float* __restrict__ center,
                                                                float* __restrict__ hand_pose) {
  __shared__ Skeleton S;
  __shared__ float sv[kMaxV * 3];
  __shared__ float sj[21][3];
  __shared__ float shift[3];
  const int t = threadIdx.x, b = blockIdx.x;
  const Layout L = layout_of(V, nc);
  pose += (size_t)b * (3 + nc), shape += (size_t)b * kShape;
  build_skeleton(S, ws, L, nc, pose, shape, hand_pose ? hand_pose + (size_t)b * kHand : nullptr);
  if (global_trans && t < kJoints * 16) {
    const int j = t / 16, e = t % 16;
    global_trans[(size_t)b * kJoints * 16 + t] = e < 12 ? S.G[j][e] : (e == 15 ? 1.0f : 0.0f);
  }
  for (int v = t; v < V; v += kThreads) {
    float vp[3], T[12];
    rest_vertex(S, ws, L, V, v, shape, vp);
    blend_vertex(S, ws, L, v, T);
    for (int r = 0; r < 3; ++r) sv[3 * v + r] = ((T[4 * r] * vp[0] + T[4 * r + 1] * vp[1]) + T[4 * r + 2] * vp[2]) + T[4 * r + 3];
  }
  __syncthreads();
  const int* tips = reinterpret_cast<const int*>(ws) + L.tips;
  if (t < 21 * 3) {
    const int i = t / 3, k = t % 3, src = joint_source(i);
    sj[i][k] = src < kJoints ? S.G[src][4 * k + 3] : sv[3 * tips[src - kJoints] + k];
  }
  __syncthreads();
  if (t < 3) {
    const bool centring = !trans && center_idx >= 0;
    shift[t] = trans ? trans[(size_t)b * 3 + t] : (centring ? -sj[center_idx][t] : 0.0f);
    if (centring && center) center[(size_t)b * 3 + t] = sj[center_idx][t];
  }
  __syncthreads();
  const bool moved = trans || center_idx >= 0;
  if (joints && t < 21 * 3) joints[(size_t)b * 63 + t] = moved ? sj[t / 3][t % 3] + shift[t % 3] : sj[t / 3][t % 3];
  if (verts)
    for (int i = t; i < 3 * V; i += kThreads) verts[(size_t)b * 3 * V + i] = moved ? sv[i] + shift[i % 3] : sv[i];
}

__global__ __launch_bounds__(kThreads) void mano_backward_kernel(const float* __restrict__ ws, int V, int nc, const float* __restrict__ pose,
                                                                 const float* __restrict__ shape, int centring, int center_idx,
                                                                 const float* __restrict__ d_verts, const float* __restrict__ d_joints,
                                                                 const float* __restrict__ d_global_trans, const float* __restrict__ d_center,
                                                                 float* __restrict__ d_pose, float* __restrict__ d_shape) {
  __shared__ Skeleton S;
  __shared__ float vp_s[kMaxV * 3];      // v_posed
  __shared__ float dv_s[kMaxV * 3];      // cotangent of the skinned vertices (before the shift)
  __shared__ float dvp_s[kMaxV * 3];     // cotangent of v_posed
  __shared__ float dj_s[21][3];          // cotangent of the 21 joints (before the shift)
  __shared__ float dA[kJoints][12];      // of the skinning transforms
  __shared__ float dGR[kJoints][9], dGt[kJoints][3], dJ[kJoints][3], dR[kJoints][9];
  __shared__ float to_root[5][15];       // what finger f hands to the root: dGR [9], dGt [3], dJ [3]
  __shared__ float dpm[kPoseMap], dbeta[kShape], dfull[48];
  const int t = threadIdx.x, b = blockIdx.x;
  const Layout L = layout_of(V, nc);
  pose += (size_t)b * (3 + nc), shape += (size_t)b * kShape;
  build_skeleton(S, ws, L, nc, pose, shape, nullptr);

  // the cotangents as given
  for (int i = t; i < 3 * V; i += kThreads) dv_s[i] = d_verts ? d_verts[(size_t)b * 3 * V + i] : 0.0f;
  if (t < 63) dj_s[t / 3][t % 3] = d_joints ? d_joints[(size_t)b * 63 + t] : 0.0f;
  __syncthreads();
  // centring: verts - c, joints - c and c itself, c = joint center_idx before the shift
  if (centring && t < 3) {
    float acc = d_center ? d_center[(size_t)b * 3 + t] : 0.0f;
    float sum = ordered_sum<16>(V, [&](int v) { return dv_s[3 * v + t]; });
    for (int i = 0; i < 21; ++i) sum += dj_s[i][t];
    dj_s[center_idx][t] += acc - sum;
  }
  __syncthreads();
  // the five tip joints are vertices
  const int* tips = reinterpret_cast<const int*>(ws) + L.tips;
  if (t < 3)
    for (int i = 0; i < 21; ++i) {
      const int src = joint_source(i);
      if (src >= kJoints) dv_s[3 * tips[src - kJoints] + t] += dj_s[i][t];
    }
  __syncthreads();
  // per vertex: v_posed again, and the cotangent of v_posed through the blended rotation
  for (int v = t; v < V; v += kThreads) {
    float vp[3], T[12];
    rest_vertex(S, ws, L, V, v, shape, vp);
    blend_vertex(S, ws, L, v, T);
    const float g0 = dv_s[3 * v], g1 = dv_s[3 * v + 1], g2 = dv_s[3 * v + 2];
    for (int c = 0; c < 3; ++c) {
      vp_s[3 * v + c] = vp[c];
      dvp_s[3 * v + c] = (T[c] * g0 + T[4 + c] * g1) + T[8 + c] * g2;
    }
  }
  __syncthreads();
  // sums over the vertices, one owner each, vertices in index order: 192 entries of the transform adjoint, 10 of the shape
  if (t < kAdj) {
    const int j = t / 12, r = (t % 12) / 4, c = t % 4;
    const float* w = ws + L.w + j;
    dA[j][t % 12] = ordered_sum<16>(V, [&](int v) {
      const float g = w[(size_t)v * kJoints] * dv_s[3 * v + r];
      return c < 3 ? g * vp_s[3 * v + c] : g;
    });
  } else if (t < kAdj + kShape) {
    const int l = t - kAdj;
    const float* sd = ws + L.sd + l;
    dbeta[l] = ordered_sum<16>(3 * V, [&](int i) { return sd[(size_t)i * kShape] * dvp_s[i]; });
  }
  __syncthreads();
  // 135 of the pose map, meanwhile (threads 192..207) the skinning transforms' adjoint goes to the chain transforms and rest joints
  if (t < kPoseMap) {
    const float* pd = ws + L.pd + t;
    dpm[t] = ordered_sum<16>(3 * V, [&](int i) { return pd[(size_t)i * kPoseMap] * dvp_s[i]; });
  } else if (t >= kAdj && t < kAdj + kJoints) {
    const int j = t - kAdj;
    const float* ext = d_global_trans ? d_global_trans + ((size_t)b * kJoints + j) * 16 : nullptr;
    int out = -1;                                   // the output joint this chain joint is
    for (int i = 0; i < 21; ++i) out = joint_source(i) == j ? i : out;
    float at[3], gt[3];
    for (int r = 0; r < 3; ++r) {
      at[r] = dA[j][4 * r + 3];
      gt[r] = at[r] + dj_s[out][r];
      if (ext) gt[r] += ext[4 * r + 3];
      dGt[j][r] = gt[r];
      for (int c = 0; c < 3; ++c) {
        float g = dA[j][4 * r + c] - at[r] * S.J[j][c];      // A_t = G_t - G_R J
        if (ext) g += ext[4 * r + c];
        dGR[j][3 * r + c] = g;
      }
    }
    for (int c = 0; c < 3; ++c) dJ[j][c] = -((S.G[j][c] * at[0] + S.G[j][4 + c] * at[1]) + S.G[j][8 + c] * at[2]);
  }
  __syncthreads();
  // the chain's adjoint from the tips to the root: thread f walks finger f inwards
  if (t < 5) {
    for (int j = 3 * t + 3; j >= 3 * t + 1; --j) {
      const int p = parent_of(j);
      float GRp[9], g[9], gt[3], rel[3], Rj[9];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) GRp[3 * r + c] = S.G[p][4 * r + c];
      for (int i = 0; i < 9; ++i) g[i] = dGR[j][i], Rj[i] = S.R[j][i];
      for (int i = 0; i < 3; ++i) gt[i] = dGt[j][i], rel[i] = S.J[j][i] - S.J[p][i];
      // G_R[j] = G_R[p] R[j]; G_t[j] = G_R[p] rel + G_t[p]
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) dR[j][3 * r + c] = (GRp[r] * g[c] + GRp[3 + r] * g[3 + c]) + GRp[6 + r] * g[6 + c];
      float up[9], back[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          up[3 * r + c] = ((g[3 * r] * Rj[3 * c] + g[3 * r + 1] * Rj[3 * c + 1]) + g[3 * r + 2] * Rj[3 * c + 2]) + gt[r] * rel[c];
      for (int c = 0; c < 3; ++c) back[c] = (GRp[c] * gt[0] + GRp[3 + c] * gt[1]) + GRp[6 + c] * gt[2];
      for (int c = 0; c < 3; ++c) dJ[j][c] += back[c];
      if (p > 0) {
        for (int i = 0; i < 9; ++i) dGR[p][i] += up[i];
        for (int i = 0; i < 3; ++i) dGt[p][i] += gt[i], dJ[p][i] -= back[i];
      } else {
        for (int i = 0; i < 9; ++i) to_root[t][i] = up[i];
        for (int i = 0; i < 3; ++i) to_root[t][9 + i] = gt[i], to_root[t][12 + i] = -back[i];
      }
    }
  }
  __syncthreads();
  if (t < 15) {          // the root takes the five fingers in their order; G[0] = [R[0] | J[0]]
    float acc = t < 9 ? dGR[0][t] : (t < 12 ? dGt[0][t - 9] : dJ[0][t - 12]);
    for (int f = 0; f < 5; ++f) acc += to_root[f][t];
    if (t < 9) dR[0][t] = acc;
    else if (t < 12) dGt[0][t - 9] = acc;
    else dJ[0][t - 12] = acc;
  }
  __syncthreads();
  if (t < 3) dJ[0][t] += dGt[0][t];
  __syncthreads();
  // rotations -> axis-angle values; rest joints -> shape
  if (t < kJoints) {
    float a[3] = {S.full[3 * t], S.full[3 * t + 1], S.full[3 * t + 2]}, d[9], da[3];
    for (int i = 0; i < 9; ++i) d[i] = t > 0 ? dR[t][i] + dpm[9 * (t - 1) + i] : dR[0][i];
    rodrigues_adjoint(a, d, da);
    for (int i = 0; i < 3; ++i) dfull[3 * t + i] = da[i];
  } else if (t >= 64 && t < 64 + kShape) {
    const int l = t - 64;
    float acc = 0.0f;
    for (int jk = 0; jk < kJoints * 3; ++jk) acc += ws[L.js + (size_t)jk * kShape + l] * dJ[jk / 3][jk % 3];
    d_shape[(size_t)b * kShape + l] = dbeta[l] + acc;
  }
  __syncthreads();
  if (t < 3) d_pose[(size_t)b * (3 + nc) + t] = dfull[t];
  else if (t < 3 + nc) {
    float acc = 0.0f;
    for (int k = 0; k < kHand; ++k) acc += ws[L.comps + (size_t)(t - 3) * kHand + k] * dfull[3 + k];
    d_pose[(size_t)b * (3 + nc) + t] = acc;
  }
}

int check_model(const void* ws, size_t ws_bytes, int32_t V, int32_t nc) {
  if (V < 1 || V > kMaxV || nc < 1 || nc > kHand || !ws || ((uintptr_t)ws & 15)) return ASDF_EINVAL;
  return ws_bytes < 4 * layout_of(V, nc).words ? ASDF_ENOSPC : ASDF_OK;
}

}  // namespace
}  // namespace asdf

using namespace asdf;

extern "C" {

int asdf_mano_workspace_bytes(int32_t num_verts, int32_t ncomps, size_t* bytes) {
  if (!bytes || num_verts < 1 || num_verts > kMaxV || ncomps < 1 || ncomps > kHand) return ASDF_EINVAL;
  *bytes = 4 * layout_of(num_verts, ncomps).words;
  return ASDF_OK;
}

int asdf_mano_prepare(int32_t num_verts, int32_t ncomps, const float* v_template_dev, const float* shapedirs_dev, const float* posedirs_dev,
                      const float* j_regressor_dev, const float* weights_dev, const float* hands_mean_dev, const float* comps_dev,
                      const int32_t* tips_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  ASDF_TRY(check_model(workspace_dev, workspace_bytes, num_verts, ncomps));
  if (!v_template_dev || !shapedirs_dev || !posedirs_dev || !j_regressor_dev || !weights_dev || !hands_mean_dev || !comps_dev || !tips_dev)
    return ASDF_EINVAL;
  if (((uintptr_t)v_template_dev | (uintptr_t)shapedirs_dev | (uintptr_t)posedirs_dev | (uintptr_t)j_regressor_dev | (uintptr_t)weights_dev |
       (uintptr_t)hands_mean_dev | (uintptr_t)comps_dev | (uintptr_t)tips_dev) & 3)
    return ASDF_EINVAL;
  hipLaunchKernelGGL(mano_prepare_kernel, dim3(64), dim3(kThreads), 0, (hipStream_t)stream, (int)num_verts, (int)ncomps, v_template_dev,
                     shapedirs_dev, posedirs_dev, j_regressor_dev, weights_dev, hands_mean_dev, comps_dev, (const int*)tips_dev,
                     reinterpret_cast<float*>(workspace_dev));
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_mano_forward(const void* workspace_dev, size_t workspace_bytes, int32_t num_verts, int32_t ncomps, int32_t B, const float* pose_dev,
                      const float* shape_dev, const float* trans_dev, int32_t center_idx, float* verts_dev, float* joints_dev,
                      float* global_trans_dev, float* center_dev, float* hand_pose_dev, void* stream) {
  ASDF_TRY(check_model(workspace_dev, workspace_bytes, num_verts, ncomps));
  if (B < 0 || center_idx < -1 || center_idx > 20 || (B > 0 && (!pose_dev || !shape_dev))) return ASDF_EINVAL;
  if (((uintptr_t)pose_dev | (uintptr_t)shape_dev | (uintptr_t)trans_dev | (uintptr_t)verts_dev | (uintptr_t)joints_dev |
       (uintptr_t)global_trans_dev | (uintptr_t)center_dev | (uintptr_t)hand_pose_dev) & 3)
    return ASDF_EINVAL;
  if (B == 0 || (!verts_dev && !joints_dev && !global_trans_dev && !center_dev && !hand_pose_dev)) return ASDF_OK;
  hipLaunchKernelGGL(mano_forward_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float*>(workspace_dev), (int)num_verts, (int)ncomps, pose_dev, shape_dev, trans_dev, (int)center_idx,
                     verts_dev, joints_dev, global_trans_dev, center_dev, hand_pose_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

int asdf_mano_backward(const void* workspace_dev, size_t workspace_bytes, int32_t num_verts, int32_t ncomps, int32_t B, const float* pose_dev,
                       const float* shape_dev, const float* trans_dev, int32_t center_idx, const float* d_verts_dev, const float* d_joints_dev,
                       const float* d_global_trans_dev, const float* d_center_dev, float* d_pose_dev, float* d_shape_dev, void* stream) {
  ASDF_TRY(check_model(workspace_dev, workspace_bytes, num_verts, ncomps));
  if (B < 0 || center_idx < -1 || center_idx > 20 || (B > 0 && (!pose_dev || !shape_dev || !d_pose_dev || !d_shape_dev))) return ASDF_EINVAL;
  if (((uintptr_t)pose_dev | (uintptr_t)shape_dev | (uintptr_t)trans_dev | (uintptr_t)d_verts_dev | (uintptr_t)d_joints_dev |
       (uintptr_t)d_global_trans_dev | (uintptr_t)d_center_dev | (uintptr_t)d_pose_dev | (uintptr_t)d_shape_dev) & 3)
    return ASDF_EINVAL;
  if (B == 0) return ASDF_OK;
  const int centring = !trans_dev && center_idx >= 0;
  hipLaunchKernelGGL(mano_backward_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float*>(workspace_dev), (int)num_verts, (int)ncomps, pose_dev, shape_dev, centring, (int)center_idx,
                     d_verts_dev, d_joints_dev, d_global_trans_dev, centring ? d_center_dev : nullptr, d_pose_dev, d_shape_dev);
  ASDF_HIP(hipGetLastError());
  return ASDF_OK;
}

}  // extern "C"
