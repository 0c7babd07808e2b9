// Three-point hypotheses scored against every match, and the best few selected (gfx950): the third step of the global registration
// (ops/cloud.py cloud_ransac, atvsnet/register_cloud.py global_init).  The definition is in include/atvsnet_hip.h;
// tests/cloud_global_restated.py restates it operation for operation.  Built with -ffp-contract=off.  No atomics.
//
// ONE LANE PER HYPOTHESIS, in double.  The matrix comes from two orthonormal frames (Gram-Schmidt of two edges and their cross
// product), the ratio of the perimeters and the centroids: no SVD, no iteration, 12 doubles in named registers.  The c pairs pass
// through LDS in tiles of 256 (one pair per thread, 24 bytes); in the scoring loop every lane reads the same address, a broadcast.
// A lane writes its count (int32) and its sum (double); the matrix is formed again, by the same function, for the few that win.
//
// THE SELECTION is one workgroup and `best` rounds.  A round finds the first key of the order (larger count, smaller sum, lower
// index) that comes strictly after the previous round's winner: every thread walks its hypotheses i = thread, thread + 256, ..., the
// 64 lanes fold as the moments' tree does (lane j takes lane j + 32, + 16, .. + 1), the four wavefronts as (w0, w1), (w2, w3).  The
// order is total (the index breaks every tie), so the winner is a function of the keys alone.
#include <math.h>

#include "common.h"
#include "cloud_common.h"

namespace {

constexpr int kMaxBest = ATVS_CLOUD_RANSAC_MAX_BEST;
constexpr long kMaxHypotheses = 1L << 24;
constexpr double kMinEdge2 = ATVS_CLOUD_RANSAC_MIN_EDGE2;
constexpr double kMinSin2 = 1e-12;
constexpr int kOutWords = 15;

struct Frame {
  double X[3], Y[3], Z[3], L[3], G[3];
  bool ok;
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ Frame triangle_frame(const float* __restrict__ P, int i0, int i1, int i2) {
  Frame f;
  double x0[3], x1[3], x2[3], p[3], q[3], r[3], z[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    x0[a] = (double)P[(long)i0 * 3 + a];
    x1[a] = (double)P[(long)i1 * 3 + a];
    x2[a] = (double)P[(long)i2 * 3 + a];
    p[a] = x1[a] - x0[a];
    q[a] = x2[a] - x0[a];
    r[a] = x2[a] - x1[a];
    f.G[a] = ((x0[a] + x1[a]) + x2[a]) / 3.0;
  }
  const double pp = dot3(p, p), qq = dot3(q, q), rr = dot3(r, r);
  f.L[0] = sqrt(pp);
  f.L[1] = sqrt(qq);
  f.L[2] = sqrt(rr);
#pragma unroll
  for (int a = 0; a < 3; ++a) f.X[a] = p[a] / f.L[0];
  const double qx = dot3(q, f.X);
#pragma unroll
  for (int a = 0; a < 3; ++a) z[a] = q[a] - qx * f.X[a];
  const double zz = dot3(z, z);
  const double zl = sqrt(zz);
#pragma unroll
  for (int a = 0; a < 3; ++a) f.Y[a] = z[a] / zl;
  f.Z[0] = f.X[1] * f.Y[2] - f.X[2] * f.Y[1];
  f.Z[1] = f.X[2] * f.Y[0] - f.X[0] * f.Y[2];
  f.Z[2] = f.X[0] * f.Y[1] - f.X[1] * f.Y[0];
  f.ok = (pp >= kMinEdge2) & (qq >= kMinEdge2) & (rr >= kMinEdge2) & (zz > kMinSin2 * qq);      // a NaN fails each
  return f;
}

// The hypothesis of one triple -> M (3 x 4, row-major); false: invalid.
__device__ __forceinline__ bool hypothesis(const float* __restrict__ src, const float* __restrict__ dst, long c, const int* __restrict__ triple,
                                           int with_scale, double edge_ratio, double* M) {
  const int i0 = triple[0], i1 = triple[1], i2 = triple[2];
  const bool in = (i0 >= 0) & (i1 >= 0) & (i2 >= 0) & ((long)i0 < c) & ((long)i1 < c) & ((long)i2 < c) & (i0 != i1) & (i0 != i2) & (i1 != i2);
  if (!in) return false;
  const Frame s = triangle_frame(src, i0, i1, i2), d = triangle_frame(dst, i0, i1, i2);
  const double scale = with_scale ? ((d.L[0] + d.L[1]) + d.L[2]) / ((s.L[0] + s.L[1]) + s.L[2]) : 1.0;
  bool ok = s.ok & d.ok;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double sl = scale * s.L[e];
    ok = ok & (d.L[e] >= edge_ratio * sl) & (edge_ratio * d.L[e] <= sl);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int col = 0; col < 3; ++col) M[r * 4 + col] = scale * ((d.X[r] * s.X[col] + d.Y[r] * s.Y[col]) + d.Z[r] * s.Z[col]);
    M[r * 4 + 3] = d.G[r] - ((M[r * 4 + 0] * s.G[0] + M[r * 4 + 1] * s.G[1]) + M[r * 4 + 2] * s.G[2]);
  }
  return ok;
}

__global__ __launch_bounds__(kThreads) void cloud_ransac_score_kernel(const float* __restrict__ src, const float* __restrict__ dst, long c,
                                                                      const int* __restrict__ triples, long h, double tau, int with_scale,
                                                                      double edge_ratio, int* __restrict__ counts, double* __restrict__ sums) {
  __shared__ float tile[kThreads * 6];
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  double M[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) M[e] = 0.0;
  const bool valid = j < h ? hypothesis(src, dst, c, triples + j * 3, with_scale, edge_ratio, M) : false;      // every lane stays for the barriers
  const double tau2 = tau * tau;
  int count = 0;
  double sum = 0.0;
  for (long base = 0; base < c; base += kThreads) {
    const int rows = (int)(c - base < (long)kThreads ? c - base : (long)kThreads);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        tile[threadIdx.x * 6 + a] = src[(base + threadIdx.x) * 3 + a];
        tile[threadIdx.x * 6 + 3 + a] = dst[(base + threadIdx.x) * 3 + a];
      }
    }
    __syncthreads();
    if (!valid) continue;
    for (int i = 0; i < rows; ++i) {
      const double x0 = (double)tile[i * 6 + 0], x1 = (double)tile[i * 6 + 1], x2 = (double)tile[i * 6 + 2];
      const double e0 = (((M[0] * x0 + M[1] * x1) + M[2] * x2) + M[3]) - (double)tile[i * 6 + 3];
      const double e1 = (((M[4] * x0 + M[5] * x1) + M[6] * x2) + M[7]) - (double)tile[i * 6 + 4];
      const double e2 = (((M[8] * x0 + M[9] * x1) + M[10] * x2) + M[11]) - (double)tile[i * 6 + 5];
      const double d = (e0 * e0 + e1 * e1) + e2 * e2;
      if (d <= tau2) {
        count += 1;
        sum = sum + d;
      }
    }
  }
  if (j < h) {
    counts[j] = valid ? count : -1;
    sums[j] = valid ? sum : 0.0;
  }
}

struct Key {
  int count;                                           // -1: none
  double sum;
  int index;
};

// a before b in the order: larger count, smaller sum, lower index
__device__ __forceinline__ bool before(const Key& a, const Key& b) {
  return (a.count > b.count) | ((a.count == b.count) & ((a.sum < b.sum) | ((a.sum == b.sum) & (a.index < b.index))));
}

__device__ __forceinline__ Key first_of(const Key& a, const Key& b) { return before(b, a) ? b : a; }

__global__ __launch_bounds__(kThreads) void cloud_ransac_select_kernel(const float* __restrict__ src, const float* __restrict__ dst, long c,
                                                                       const int* __restrict__ triples, long h, int with_scale, double edge_ratio,
                                                                       const int* __restrict__ counts, const double* __restrict__ sums, int best,
                                                                       unsigned long long* __restrict__ out) {
  __shared__ Key wave[kThreads / 64];
  __shared__ Key winner;
  const Key none = {-1, 0.0, 0x7fffffff};
  Key prev = {0x7fffffff, 0.0, -1};                     // before every hypothesis
  for (int round = 0; round < best; ++round) {
    Key mine = none;
    for (long i = threadIdx.x; i < h; i += kThreads) {
      const Key k = {counts[i], sums[i], (int)i};
      if (k.count >= 0 && before(prev, k)) mine = first_of(mine, k);
    }
    for (int off = 32; off > 0; off >>= 1) {
      const Key o = {__shfl_down(mine.count, off), __shfl_down(mine.sum, off), __shfl_down(mine.index, off)};
      mine = first_of(mine, o);
    }
    if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      const Key w = first_of(first_of(wave[0], wave[1]), first_of(wave[2], wave[3]));
      winner = w;
      double M[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) M[e] = 0.0;
      if (w.count >= 0) hypothesis(src, dst, c, triples + (long)w.index * 3, with_scale, edge_ratio, M);
      unsigned long long* slot = out + (long)round * kOutWords;
#pragma unroll
      for (int e = 0; e < 12; ++e) slot[e] = (unsigned long long)__double_as_longlong(w.count >= 0 ? M[e] : 0.0);
      slot[12] = (unsigned long long)(long long)w.count;
      slot[13] = (unsigned long long)__double_as_longlong(w.count >= 0 ? w.sum : 0.0);
      slot[14] = (unsigned long long)(long long)(w.count >= 0 ? w.index : -1);
    }
    __syncthreads();
    prev = winner;
    if (prev.count < 0) prev.index = 0x7fffffff;        // nothing is left: every later round finds none as well
    __syncthreads();                                    // `wave` and `winner` are rewritten in the next round
  }
}

}  // namespace

extern "C" int atvs_cloud_ransac_scratch_size(long h, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (h < 1 || h > kMaxHypotheses) return ATVS_ERR_SHAPE;
  *bytes = (long)(align256((size_t)h * 4) + align256((size_t)h * 8));
  return ATVS_OK;
}

extern "C" int atvs_cloud_ransac_score(const float* src, const float* dst, long c, const int* triples, long h, double tau, int with_scale,
                                       double edge_ratio, int best, void* scratch, long scratch_bytes, void* out, atvs_stream_t stream) {
  long need = 0;
  if (c < 3 || c > kMaxPoints || h < 1 || h > kMaxHypotheses) return ATVS_ERR_SHAPE;
  if (!(tau > 0.0) || !(tau < (double)__builtin_huge_valf()) || !(edge_ratio > 0.0 && edge_ratio <= 1.0)) return ATVS_ERR_ARG;
  if ((with_scale != 0 && with_scale != 1) || best < 1 || best > kMaxBest) return ATVS_ERR_ARG;
  if (atvs_cloud_ransac_scratch_size(h, &need) != ATVS_OK || scratch_bytes < need) return ATVS_ERR_SHAPE;
  if (!src || !dst || !triples || !scratch || !out) return ATVS_ERR_NULL;
  int* counts = static_cast<int*>(scratch);
  double* sums = reinterpret_cast<double*>(static_cast<char*>(scratch) + align256((size_t)h * 4));
  hipLaunchKernelGGL(cloud_ransac_score_kernel, dim3((unsigned)cdiv(h, kThreads)), dim3(kThreads), 0, as_stream(stream), src, dst, c, triples, h,
                     tau, with_scale, edge_ratio, counts, sums);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_ransac_select_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), src, dst, c, triples, h, with_scale, edge_ratio,
                     (const int*)counts, (const double*)sums, best, static_cast<unsigned long long*>(out));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
