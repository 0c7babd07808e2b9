// FPFH descriptors and their nearest neighbour in feature space (gfx950): the first two steps of the global registration
// (ops/cloud.py cloud_fpfh / cloud_feature_nearest, atvsnet/register_cloud.py global_init).  The definitions are in
// include/atvsnet_hip.h; tests/cloud_global_restated.py restates them operation for operation.  Built with -ffp-contract=off: every
// operation below is rounded on its own.  No atomics, no transcendental function; a row's output depends on its inputs alone.
//
// FPFH, TWO LAUNCHES, ONE LANE PER POINT.  The first walks the point's row of idx twice (the centroid direction that fixes the
// normal's sign, then the pairs) and gathers k x 24 bytes each time; its three histograms are integer counts of at most k <= 32, kept
// in 8-bit fields of six 64-bit registers (nothing is indexed at run time) and written as ONE ROW OF 36 BYTES: 33 counts, the number
// of counting pairs, two zero bytes.  The second launch gathers k such rows per lane -- k x 36 bytes instead of the k x 132 a float
// histogram would be, nine 4-byte loads per neighbour that stay in L2 for a down-sampled cloud (50k points: 1.8 MB) -- and weights
// them in 33 named double accumulators.  Rows are read by the lane that needs them; nothing is staged through LDS, since neighbouring
// lanes share rows only as far as the voxel order keeps neighbours together.  No time is measured here; the two launches are not
// fused because the second needs every row of the first.
//
// FEATURE NEAREST: each lane owns one query (33 floats in registers); reference rows pass through LDS in tiles of
// ATVS_CLOUD_FEATURE_TILE rows padded to 36 floats (16-byte rows: eight 16-byte reads and one 4-byte read per row; every lane reads
// the same address, a broadcast without bank conflicts).  Rows are taken in ascending index and only a strictly smaller distance
// replaces the best, so the lowest index wins a tie.
#include <math.h>

#include "common.h"
#include "cloud_common.h"

namespace {

constexpr int kMaxK = ATVS_CLOUD_MAX_K;
constexpr int kBins = ATVS_CLOUD_FPFH_BINS;
constexpr int kFeat = 3 * kBins;                       // 33
constexpr int kRowWords = 9;                           // 36 bytes: 33 counts, the pair count, two zero bytes
constexpr int kTile = ATVS_CLOUD_FEATURE_TILE;
constexpr int kRowPad = 36;                            // floats per reference row in LDS
__constant__ double kThetaCos[10] = ATVS_CLOUD_FPFH_THETA_COS;
__constant__ double kThetaSin[10] = ATVS_CLOUD_FPFH_THETA_SIN;

static_assert(kBins == 11 && kMaxK < 256, "a count and the pair count fit a byte; 11 bins fill 8 + 3 fields");

// the number of the ten edges (2 e - 11) / 11 at or below v: a tie goes to the upper bin
__device__ __forceinline__ int linear_bin(double v) {
  const double v11 = 11.0 * v;
  int b = 0;
#pragma unroll
  for (int e = 1; e <= 10; ++e) b += (v11 >= (double)(2 * e - 11)) ? 1 : 0;
  return b;
}

__device__ __forceinline__ int theta_bin(double x, double y) {
  int b = 0;
#pragma unroll
  for (int e = 0; e < 10; ++e) b += (kThetaCos[e] * y - kThetaSin[e] * x >= 0.0) ? 1 : 0;
  return b;
}

struct Hist {                                          // 11 counts in 8-bit fields
  unsigned long long lo, hi;
  __device__ __forceinline__ void add(int b) {
    lo += b < 8 ? 1ull << (8 * b) : 0ull;
    hi += b < 8 ? 0ull : 1ull << (8 * (b - 8));
  }
  __device__ __forceinline__ unsigned get(int b) const { return (unsigned)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 255ull); }
};

__device__ __forceinline__ unsigned row_byte(const unsigned* w, int b) { return (w[b >> 2] >> (8 * (b & 3))) & 255u; }

__global__ __launch_bounds__(kThreads) void cloud_spfh_kernel(const float* __restrict__ points, long n, const int* __restrict__ idx, int k,
                                                              const float* __restrict__ normals, unsigned* __restrict__ rows) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const float pxf = points[j * 3 + 0], pyf = points[j * 3 + 1], pzf = points[j * 3 + 2];
  const float nxf = normals[j * 3 + 0], nyf = normals[j * 3 + 1], nzf = normals[j * 3 + 2];
  const double px = (double)pxf, py = (double)pyf, pz = (double)pzf;
  const double n0 = (double)nxf, n1 = (double)nyf, n2 = (double)nzf;
  const bool own = finite3(pxf, pyf, pzf) & finite3(nxf, nyf, nzf) & ((n0 * n0 + n1 * n1) + n2 * n2 > 0.0);
  const int* __restrict__ row = idx + j * k;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  for (int t = 0; t < k; ++t) {
    const int i = row[t];
    if (i < 0 || (long)i >= n) continue;
    const float qx = points[(long)i * 3 + 0], qy = points[(long)i * 3 + 1], qz = points[(long)i * 3 + 2];
    if (!finite3(qx, qy, qz)) continue;
    c0 = c0 + ((double)qx - px);
    c1 = c1 + ((double)qy - py);
    c2 = c2 + ((double)qz - pz);
  }
  const double turn = ((n0 * c0 + n1 * c1) + n2 * c2 < 0.0) ? -1.0 : 1.0;              // an exact product with +-1
  const double u0 = n0 * turn, u1 = n1 * turn, u2 = n2 * turn;
  Hist ha = {0ull, 0ull}, hp = {0ull, 0ull}, ht = {0ull, 0ull};
  unsigned pairs = 0;
  for (int t = 0; t < k; ++t) {
    const int i = row[t];
    if (i < 0 || (long)i >= n) continue;
    const float qx = points[(long)i * 3 + 0], qy = points[(long)i * 3 + 1], qz = points[(long)i * 3 + 2];
    const float mxf = normals[(long)i * 3 + 0], myf = normals[(long)i * 3 + 1], mzf = normals[(long)i * 3 + 2];
    double m0 = (double)mxf, m1 = (double)myf, m2 = (double)mzf;
    const double d0 = (double)qx - px, d1 = (double)qy - py, d2 = (double)qz - pz;
    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
    const double g0 = u1 * d2 - u2 * d1, g1 = u2 * d0 - u0 * d2, g2 = u0 * d1 - u1 * d0;
    const double gg = (g0 * g0 + g1 * g1) + g2 * g2;
    const bool counts = own & finite3(qx, qy, qz) & finite3(mxf, myf, mzf) & ((m0 * m0 + m1 * m1) + m2 * m2 > 0.0) & (dd > 0.0) & (gg > 0.0);
    if (!counts) continue;
    const double side = ((u0 * m0 + u1 * m1) + u2 * m2 < 0.0) ? -1.0 : 1.0;
    m0 = m0 * side;
    m1 = m1 * side;
    m2 = m2 * side;
    const double gl = sqrt(gg);
    const double v0 = g0 / gl, v1 = g1 / gl, v2 = g2 / gl;
    const double w0 = u1 * v2 - u2 * v1, w1 = u2 * v0 - u0 * v2, w2 = u0 * v1 - u1 * v0;
    const double alpha = (v0 * m0 + v1 * m1) + v2 * m2;
    const double phi = ((u0 * d0 + u1 * d1) + u2 * d2) / sqrt(dd);
    const double x = (u0 * m0 + u1 * m1) + u2 * m2, y = (w0 * m0 + w1 * m1) + w2 * m2;
    ha.add(linear_bin(alpha));
    hp.add(linear_bin(phi));
    ht.add(theta_bin(x, y));
    pairs += 1;
  }
  unsigned w[kRowWords];
#pragma unroll
  for (int q = 0; q < kRowWords; ++q) {
    unsigned word = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int b = 4 * q + s;
      const unsigned v = b < kBins ? ha.get(b) : (b < 2 * kBins ? hp.get(b - kBins) : (b < kFeat ? ht.get(b - 2 * kBins) : (b == kFeat ? pairs : 0u)));
      word |= v << (8 * s);
    }
    w[q] = word;
  }
#pragma unroll
  for (int q = 0; q < kRowWords; ++q) rows[j * kRowWords + q] = w[q];
}

__global__ __launch_bounds__(kThreads) void cloud_fpfh_kernel(const float* __restrict__ points, long n, const int* __restrict__ idx, int k,
                                                              const unsigned* __restrict__ rows, float* __restrict__ out) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  unsigned w[kRowWords];
#pragma unroll
  for (int q = 0; q < kRowWords; ++q) w[q] = rows[j * kRowWords + q];
  const unsigned cj = row_byte(w, kFeat);
  float* __restrict__ o = out + j * kFeat;
  if (cj == 0) {
#pragma unroll
    for (int b = 0; b < kFeat; ++b) o[b] = 0.0f;
    return;
  }
  double g[kFeat];                                      // the neighbours' weighted sum; the point's own part joins at the end
#pragma unroll
  for (int b = 0; b < kFeat; ++b) g[b] = 0.0;
  const double px = (double)points[j * 3 + 0], py = (double)points[j * 3 + 1], pz = (double)points[j * 3 + 2];
  const int* __restrict__ row = idx + j * k;
  for (int t = 0; t < k; ++t) {
    const int i = row[t];
    if (i < 0 || (long)i >= n) continue;
    const float qx = points[(long)i * 3 + 0], qy = points[(long)i * 3 + 1], qz = points[(long)i * 3 + 2];
    if (!finite3(qx, qy, qz)) continue;
    const double d0 = (double)qx - px, d1 = (double)qy - py, d2 = (double)qz - pz;
    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!(dd > 0.0)) continue;
    unsigned v[kRowWords];
#pragma unroll
    for (int q = 0; q < kRowWords; ++q) v[q] = rows[(long)i * kRowWords + q];
    const unsigned ci = row_byte(v, kFeat);
    if (ci == 0) continue;
    const double r = 1.0 / ((double)ci * dd);
#pragma unroll
    for (int b = 0; b < kFeat; ++b) g[b] = g[b] + (double)row_byte(v, b) * r;
  }
#pragma unroll
  for (int part = 0; part < 3; ++part) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < kBins; ++b) s = s + g[part * kBins + b];
#pragma unroll
    for (int b = 0; b < kBins; ++b) {
      const double own = (double)row_byte(w, part * kBins + b) / (double)cj;
      o[part * kBins + b] = s > 0.0 ? (float)((own + g[part * kBins + b] / s) * 0.5) : (float)own;
    }
  }
}

__global__ __launch_bounds__(kThreads) void cloud_feature_nearest_kernel(const float* __restrict__ ref, long n, const float* __restrict__ query,
                                                                         long m, float* __restrict__ d2, int* __restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float tile[kTile * kRowPad];
  __shared__ int is_zero[kTile];
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = j < m;                              // every lane stays for the loads and the barriers
  float q[kFeat];
  bool any = false;
#pragma unroll
  for (int b = 0; b < kFeat; ++b) {
    q[b] = live ? query[j * kFeat + b] : 0.0f;
    any = any | (q[b] != 0.0f);
  }
  float best = __uint_as_float(0x7f800000u);
  int at = -1;
  for (long base = 0; base < n; base += kTile) {
    const int count = (int)(n - base < (long)kTile ? n - base : (long)kTile);
    __syncthreads();                                    // the previous tile has been read
    for (int e = threadIdx.x; e < count * kFeat; e += kThreads) {
      const int r = e / kFeat;
      tile[r * kRowPad + (e - r * kFeat)] = ref[base * kFeat + e];
    }
    __syncthreads();
    if ((int)threadIdx.x < count) {
      bool z = true;
      for (int b = 0; b < kFeat; ++b) z = z & (tile[threadIdx.x * kRowPad + b] == 0.0f);
      is_zero[threadIdx.x] = z ? 1 : 0;
    }
    __syncthreads();
    if (!(live && any)) continue;
    for (int r = 0; r < count; ++r) {
      if (is_zero[r]) continue;
      const float4* __restrict__ rp = reinterpret_cast<const float4*>(tile + r * kRowPad);
      float acc = 0.0f;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float4 v = rp[g];
        const float e0 = q[4 * g + 0] - v.x, e1 = q[4 * g + 1] - v.y, e2 = q[4 * g + 2] - v.z, e3 = q[4 * g + 3] - v.w;
        acc = g == 0 ? e0 * e0 : acc + e0 * e0;
        acc = acc + e1 * e1;
        acc = acc + e2 * e2;
        acc = acc + e3 * e3;
      }
      const float e32 = q[32] - tile[r * kRowPad + 32];
      acc = acc + e32 * e32;
      if (acc < best) {                                 // strictly: the lowest index keeps a tie; a NaN never wins
        best = acc;
        at = (int)(base + r);
      }
    }
  }
  if (live) {
    d2[j] = best;
    idx[j] = at;
  }
}

}  // namespace

extern "C" int atvs_cloud_fpfh_scratch_size(long n, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)align256((size_t)n * kRowWords * 4 + 256);
  return ATVS_OK;
}

extern "C" int atvs_cloud_fpfh(const float* points, long n, const int* idx, int k, const float* normals, void* scratch, long scratch_bytes,
                               float* out, atvs_stream_t stream) {
  long need = 0;
  if (n < 0 || n > kMaxPoints || k < 1 || k > kMaxK) return ATVS_ERR_SHAPE;
  if (atvs_cloud_fpfh_scratch_size(n, &need) != ATVS_OK || scratch_bytes < need) return ATVS_ERR_SHAPE;
  if (n == 0) return ATVS_OK;
  if (!points || !idx || !normals || !scratch || !out) return ATVS_ERR_NULL;
  unsigned* rows = static_cast<unsigned*>(scratch);
  const dim3 grid((unsigned)cdiv(n, kThreads)), block(kThreads);
  hipLaunchKernelGGL(cloud_spfh_kernel, grid, block, 0, as_stream(stream), points, n, idx, k, normals, rows);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_fpfh_kernel, grid, block, 0, as_stream(stream), points, n, idx, k, (const unsigned*)rows, out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_cloud_feature_nearest(const float* ref, long n, const float* query, long m, float* d2, int* idx, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!query || !d2 || !idx || (n > 0 && !ref)) return ATVS_ERR_NULL;
  hipLaunchKernelGGL(cloud_feature_nearest_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, as_stream(stream), ref, n, query, m,
                     d2, idx);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
