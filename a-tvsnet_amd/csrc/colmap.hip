// COLMAP model import (gfx950): the per-image depth range and the co-visibility matrix of atvsnet/colmap.py.
//
// atvs_colmap_depth_range restates ColmapSparse.estimate_max_disparities (atvsnet/colmap_helpers.py:317-331): every 3-D point is
// projected into every image in float64 and the disparities d = 1 / z of the points in view are ranked.  No (images x points)
// buffer exists: the rank statistics are found by a radix select over the 64-bit patterns of the disparities (positive doubles,
// +inf included, order like their bits), eight passes of 8-bit digits, each pass projecting every pair again:
//   hist    one workgroup per (run of kRun points, group of kGroup images): the points in view whose top bits match an image's
//           current prefix, counted per digit in LDS (one histogram per rank; pass 0 one for both), then added to the image's
//           global histogram with integer atomics (skipping empty bins), so the counts do not depend on the order of arrival;
//   select  one wave per image: pass 0 sums n and forms the two ranks int(n * p), int(n * (1 - p)) in double as Python does;
//           each pass walks a histogram to the bin holding the remaining rank, appends its digit to the prefix and clears the
//           histogram for the next pass.  After pass 7 the prefix IS the order statistic.
// atvs_colmap_covisibility restates generate_neighbor_list's set intersections (colmap_helpers.py:333-347): one wave per track
// (the distinct images observing one 3-D point), its L * (L - 1) ordered pairs spread over the 64 lanes, one integer atomic add
// per pair into the (images x images) matrix.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 8;              // images per workgroup of the histogram pass
constexpr int kRun = 4096;             // points per workgroup of the histogram pass
constexpr int kBins = 256;             // 8-bit digits
constexpr int kPasses = 8;             // 64 bits
constexpr int kCam = 18;               // R (3x3 row-major), t (3), fx, fy, cx, cy, width, height
constexpr int kMaxCovisImages = 16384; // 16384^2 int32 = 1 GiB

struct RangeState {                    // per image, in the scratch
  unsigned long long prefix[2];        // digits found so far of rank 0 (int(n * (1 - p))) and rank 1 (int(n * p))
  int rank[2];                         // rank still to find below the prefix
  int n;                               // points in view
  int pad;
};

__host__ __device__ inline size_t state_bytes(int n_images) { return (((size_t)n_images * sizeof(RangeState)) + 255) & ~(size_t)255; }
__host__ __device__ inline size_t scratch_bytes_for(int n_images) {
  return state_bytes(n_images) + (size_t)n_images * 2 * kBins * sizeof(unsigned);
}

// colmap_helpers.py:322-326, its order made explicit: c_k = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k, x = (c_0 / c_2) fx + cx,
// y = (c_1 / c_2) fy + cy, d = 1 / c_2; in view when 0 <= x < width, 0 <= y < height and d > 0 (NaN fails every comparison).
__device__ __forceinline__ bool project(const double* __restrict__ c, double X, double Y, double Z, double* d) {
  const double c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9];
  const double c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10];
  const double c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11];
  const double x = (c0 / c2) * c[12] + c[14];
  const double y = (c1 / c2) * c[13] + c[15];
  *d = 1.0 / c2;
  return x >= 0.0 && x < c[16] && y >= 0.0 && y < c[17] && *d > 0.0;
}

__global__ __launch_bounds__(kThreads) void range_hist_kernel(const double* __restrict__ pts, int n_points,
                                                              const double* __restrict__ cams, int n_images, int pass,
                                                              const RangeState* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned h[kGroup * 2 * kBins];
  __shared__ double cam[kGroup * kCam];
  __shared__ unsigned long long prefix[kGroup * 2];
  const int g0 = blockIdx.y * kGroup;
  const int ng = min(kGroup, n_images - g0);
  for (int i = threadIdx.x; i < kGroup * 2 * kBins; i += kThreads) h[i] = 0u;
  for (int i = threadIdx.x; i < ng * kCam; i += kThreads) cam[i] = cams[(size_t)g0 * kCam + i];
  if ((int)threadIdx.x < ng * 2) prefix[threadIdx.x] = pass == 0 ? 0ull : state[g0 + (threadIdx.x >> 1)].prefix[threadIdx.x & 1];
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const unsigned long long mask = pass == 0 ? 0ull : (~0ull << (64 - 8 * pass));
  const int p0 = blockIdx.x * kRun;
  const int p1 = min(n_points, p0 + kRun);
  for (int p = p0 + (int)threadIdx.x; p < p1; p += kThreads) {
    const double X = pts[(size_t)p * 3 + 0], Y = pts[(size_t)p * 3 + 1], Z = pts[(size_t)p * 3 + 2];
    for (int g = 0; g < ng; ++g) {
      double d;
      if (!project(cam + g * kCam, X, Y, Z, &d)) continue;
      const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
      const unsigned bin = (unsigned)(bits >> shift) & (kBins - 1);
      unsigned* hg = h + g * 2 * kBins;
      if ((bits & mask) == prefix[g * 2 + 0]) atomicAdd(hg + bin, 1u);
      if (pass > 0 && (bits & mask) == prefix[g * 2 + 1]) atomicAdd(hg + kBins + bin, 1u);
    }
  }
  __syncthreads();
  unsigned* out = hist + (size_t)g0 * 2 * kBins;
  for (int i = threadIdx.x; i < ng * 2 * kBins; i += kThreads) {
    const unsigned v = h[i];
    if (v) atomicAdd(out + i, v);
  }
}

__global__ __launch_bounds__(64) void range_select_kernel(int pass, double percentile, RangeState* __restrict__ state,
                                                          unsigned* __restrict__ hist, int* __restrict__ n_in_view,
                                                          double* __restrict__ d_lo, double* __restrict__ d_hi) {
  __shared__ unsigned cnt[2 * kBins];
  const int img = blockIdx.x;
  unsigned* hg = hist + (size_t)img * 2 * kBins;
  for (int i = threadIdx.x; i < 2 * kBins; i += 64) {
    cnt[i] = hg[i];
    hg[i] = 0u;                                             // the next pass adds into a clear histogram
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  RangeState s = state[img];
  if (pass == 0) {
    long long n = 0;
    for (int b = 0; b < kBins; ++b) n += cnt[b];
    s.n = (int)n;
    s.prefix[0] = s.prefix[1] = 0ull;
    // int(n * (1.0 - percentile)), int(n * percentile): Python's float product, truncated (kept inside [0, n - 1])
    s.rank[0] = s.n > 0 ? min(max((int)((double)s.n * (1.0 - percentile)), 0), s.n - 1) : 0;
    s.rank[1] = s.n > 0 ? min(max((int)((double)s.n * percentile), 0), s.n - 1) : 0;
  }
  if (s.n > 0) {
    const int shift = 56 - 8 * pass;
    for (int side = 0; side < 2; ++side) {
      const unsigned* c = cnt + (pass == 0 ? 0 : side) * kBins;
      unsigned r = (unsigned)s.rank[side];
      int b = 0;
      while (b < kBins - 1 && c[b] <= r) r -= c[b++];
      s.rank[side] = (int)r;
      s.prefix[side] |= (unsigned long long)b << shift;
    }
  }
  state[img] = s;
  if (pass == kPasses - 1) {
    n_in_view[img] = s.n;
    d_lo[img] = s.n > 0 ? __longlong_as_double((long long)s.prefix[0]) : 0.0;
    d_hi[img] = s.n > 0 ? __longlong_as_double((long long)s.prefix[1]) : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void covis_kernel(const int* __restrict__ offsets, const int* __restrict__ obs, int n_tracks,
                                                         int n_obs, int n_images, int* __restrict__ covis) {
  const int t = blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= n_tracks) return;
  const int b = offsets[t], e = offsets[t + 1];
  const int L = e - b;
  // a track lists distinct images: more observers than images, or a range outside obs, is a malformed CSR and adds nothing
  if (b < 0 || e > n_obs || L < 2 || L > n_images) return;
  const int pairs = L * L;                                  // L <= 16384: below 2^28
  for (int q = lane; q < pairs; q += 64) {
    const int i = q / L, j = q - i * L;
    if (i == j) continue;
    const int a = obs[b + i], c = obs[b + j];
    if ((unsigned)a >= (unsigned)n_images || (unsigned)c >= (unsigned)n_images) continue;
    atomicAdd(covis + (size_t)a * n_images + c, 1);
  }
}

}  // namespace

extern "C" int atvs_colmap_depth_range_scratch_size(int n_images, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_images <= 0 || n_images > 65535 * kGroup) return ATVS_ERR_SHAPE;
  *bytes = (long)scratch_bytes_for(n_images);
  return ATVS_OK;
}

extern "C" int atvs_colmap_depth_range(const double* points, long n_points, const double* cams, int n_images, double percentile,
                                       void* scratch, long scratch_bytes, int* n_in_view, double* d_lo, double* d_hi,
                                       atvs_stream_t stream) {
  if (!cams || !scratch || !n_in_view || !d_lo || !d_hi || (n_points > 0 && !points)) return ATVS_ERR_NULL;
  if (n_images <= 0 || n_images > 65535 * kGroup || n_points < 0 || n_points > 0x7fffffffL) return ATVS_ERR_SHAPE;
  if (scratch_bytes < (long)scratch_bytes_for(n_images)) return ATVS_ERR_SHAPE;
  if (!(percentile > 0.0 && percentile < 1.0)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  RangeState* state = static_cast<RangeState*>(scratch);
  unsigned* hist = reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + state_bytes(n_images));
  if (hipMemsetAsync(scratch, 0, scratch_bytes_for(n_images), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const dim3 grid((unsigned)cdiv(n_points, kRun), (unsigned)cdiv(n_images, kGroup));
  for (int pass = 0; pass < kPasses; ++pass) {
    if (n_points > 0) {
      hipLaunchKernelGGL(range_hist_kernel, grid, dim3(kThreads), 0, st, points, (int)n_points, cams, n_images, pass, state, hist);
      ATVS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(range_select_kernel, dim3(n_images), dim3(64), 0, st, pass, percentile, state, hist, n_in_view, d_lo, d_hi);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}

extern "C" int atvs_colmap_covisibility(const int* offsets, const int* observers, int n_tracks, int n_obs, int n_images,
                                        int* covis, atvs_stream_t stream) {
  if (n_images <= 0 || n_images > kMaxCovisImages || n_tracks < 0 || n_obs < 0) return ATVS_ERR_SHAPE;
  if (!covis || !offsets || (n_obs > 0 && !observers)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(covis, 0, (size_t)n_images * n_images * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_tracks > 0) {
    hipLaunchKernelGGL(covis_kernel, dim3((unsigned)cdiv(n_tracks, kThreads / 64)), dim3(kThreads), 0, st, offsets, observers,
                       n_tracks, n_obs, n_images, covis);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}
