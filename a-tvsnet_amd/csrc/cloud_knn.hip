// Point-cloud neighbourhoods (gfx950): the k nearest reference points within the grid's radius, the number of reference points
// inside it, the statistics of statistical outlier removal, and the bounding box of a cloud (ops/cloud.py, atvsnet/clean_cloud.py).
// The definitions are in include/atvsnet_hip.h; tests/cloud_knn_restated.py restates them with numpy.  Built with
// -ffp-contract=off; integer atomics only (the counting sort, the bounding box), so every output is a function of its inputs.
//
// THE SEARCH is cloud_grid.h's (walk, search), the one cloud.hip runs: the grid of atvs_cloud_grid_build, the queries sorted by the
// same cells, one lane per query in cell order over the 9 contiguous record runs of its 27 cells, the float32
// d2 = (dx*dx + dy*dy) + dz*dz and the key (bits(d2) << 32) | index, whose unsigned order is the order of (d2, index).  cloud.hip's
// margin argument is about pairs with (double)d2 <= R^2, so it covers every neighbour here as it covers the nearest one.
//
// THE RADIUS TEST AS A KEY.  d2 >= +0 orders as its bits do, so { d2 : (double)d2 <= R^2 } is { d2 : bits(d2) <= bits(r2f) } with r2f
// the largest float32 whose double is <= R^2 (the header's r2 rounded to float32, one step down if that rounded up).  `limit` =
// (bits(r2f) + 1) << 32 is above every key that passes and at or below every key that fails.
//
// THE k BEST.  A lane keeps K >= k keys a[0] <= ... <= a[K-1] in registers, all `limit` at first.  A candidate enters when its key is
// below a[K-1] (one 64-bit compare; a candidate beyond the radius never is), by a fully unrolled compare-exchange chain
//     lo = min(a[t], x);  x = max(a[t], x);  a[t] = lo          t = 0 .. K-1
// which leaves the K smallest keys seen so far, sorted: a[] is only ever indexed by unrolled constants, so it stays in registers
// (K = 32: 64 VGPRs of keys; the compiled instances use no scratch memory).  K is compiled for 4, 8, 16, 32
// and k is served by the next K; the first k keys of the K smallest are the k smallest.  Keys are distinct (the index is the low
// word), so the set and its order do not depend on the order in which candidates arrive.  An entry still >= limit at the end is
// padding: (+inf, -1).
#include <math.h>

#include "common.h"
#include "cloud_grid.h"
#include "cloud_tree.h"

namespace {

constexpr int kMaxK = ATVS_CLOUD_MAX_K;
constexpr int kStatWords = 2;                              // a row of the statistics: count (int64) + one double

// bits of the largest float32 r2f with (double)r2f <= r2 (r2 > 0, possibly beyond the float32 range on either side)
__device__ __forceinline__ unsigned radius_bits(double r2) {
  float f = (float)r2;                                     // to nearest: +inf above the range, possibly 0 below it
  unsigned b = __float_as_uint(f);
  if ((double)f > r2) b -= 1u;                             // f > r2 > 0: the float32 below f is b - 1 (from +inf: the largest finite)
  return b;
}

template <int K>
__global__ __launch_bounds__(kThreads) void cloud_knn_kernel(const GridHeader* __restrict__ hdr, const unsigned* __restrict__ S,
                                                             const float4* __restrict__ rec, const unsigned* __restrict__ qS,
                                                             const float4* __restrict__ qrec, long m, int k, int exclude,
                                                             float* __restrict__ d2out, int* __restrict__ idxout) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const GridHeader g = *hdr;
  const float4 q = qrec[j];
  const unsigned orig = (unsigned)__float_as_int(q.w);
  const unsigned self = exclude ? orig : 0xffffffffu;      // no reference index is 2^32 - 1
  const unsigned long long limit = ((unsigned long long)radius_bits(g.r2) + 1ull) << 32;
  unsigned long long a[K];
#pragma unroll
  for (int t = 0; t < K; ++t) a[t] = limit;
  if (j < (long)qS[g.ncells]) {                            // not in the bucket of far / non-finite queries
    walk<2>(g, S, rec, q, [&](unsigned bits, unsigned i) {
      unsigned long long x = ((unsigned long long)bits << 32) | i;
      if (x < a[K - 1] && i != self) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
          const unsigned long long lo = a[t] < x ? a[t] : x;
          x = a[t] < x ? x : a[t];
          a[t] = lo;
        }
      }
    });
  }
  float* drow = d2out + (long)orig * k;
  int* irow = idxout + (long)orig * k;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (t < k) {
      const bool found = a[t] < limit;
      drow[t] = __uint_as_float(found ? (unsigned)(a[t] >> 32) : 0x7f800000u);
      irow[t] = found ? (int)(unsigned)(a[t] & 0xffffffffull) : -1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void cloud_radius_count_kernel(const GridHeader* __restrict__ hdr, const unsigned* __restrict__ S,
                                                                      const float4* __restrict__ rec, const unsigned* __restrict__ qS,
                                                                      const float4* __restrict__ qrec, long m, int exclude,
                                                                      int* __restrict__ count) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const GridHeader g = *hdr;
  const float4 q = qrec[j];
  const unsigned orig = (unsigned)__float_as_int(q.w);
  const unsigned self = exclude ? orig : 0xffffffffu;
  const unsigned rb = radius_bits(g.r2);
  int c = 0;
  if (j < (long)qS[g.ncells])
    walk<2>(g, S, rec, q, [&](unsigned bits, unsigned i) { c += (bits <= rb && i != self) ? 1 : 0; });
  count[orig] = c;
}

__global__ __launch_bounds__(kThreads) void cloud_knn_mean_kernel(const float* __restrict__ d2, long m, int k, double* __restrict__ s) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const float* row = d2 + j * k;
  const float big = __uint_as_float(0x7f800000u);
  double sum = 0.0;
  bool all = true;
  for (int t = 0; t < k; ++t) {
    const float v = row[t];
    all = all && (fabsf(v) < big);                         // +inf (padding) or NaN: the k-th neighbour is not known
    sum = sum + sqrt((double)v);
  }
  s[j] = all ? sum / (double)k : (double)big;
}

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) < (double)__uint_as_float(0x7f800000u); }

// The mean of a first-pass row (count, sum): ONE definition for the second pass and the result.
__device__ __forceinline__ double mean_of(const unsigned long long* row) {
  const long long c = (long long)row[0];
  return c > 0 ? __longlong_as_double((long long)row[1]) / (double)c : 0.0;
}

// pass 1: the count of finite entries and their sum
__global__ __launch_bounds__(kThreads) void cloud_sor_sum_kernel(const double* __restrict__ s, long m, unsigned long long* __restrict__ rows) {
  __shared__ MomentShared<kStatWords - 1> sh;
  moment_row<kStatWords - 1>(m, [&](long i, long long& cnt, double* v) {
    const double x = s[i];
    if (!finite_f64(x)) return;
    cnt += 1;
    v[0] = v[0] + x;
  }, rows, sh);
}

// pass 2: the sum of (s - mean)^2 over the finite entries; the mean is the first pass's
__global__ __launch_bounds__(kThreads) void cloud_sor_dev_kernel(const double* __restrict__ s, long m, const unsigned long long* __restrict__ first,
                                                                 unsigned long long* __restrict__ rows) {
  __shared__ MomentShared<kStatWords - 1> sh;
  const double mu = mean_of(first);
  moment_row<kStatWords - 1>(m, [&](long i, long long& cnt, double* v) {
    const double x = s[i];
    if (!finite_f64(x)) return;
    const double d = x - mu;
    cnt += 1;
    v[0] = v[0] + d * d;
  }, rows, sh);
}

__global__ void cloud_sor_result_kernel(const unsigned long long* __restrict__ first, const unsigned long long* __restrict__ second,
                                        unsigned long long* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long c = (long long)first[0];
  const double var = c >= 2 ? __longlong_as_double((long long)second[1]) / (double)(c - 1) : 0.0;
  out[0] = (unsigned long long)c;
  out[1] = (unsigned long long)__double_as_longlong(mean_of(first));
  out[2] = (unsigned long long)__double_as_longlong(c >= 2 ? sqrt(var) : 0.0);
}

// box (6 words of cloud_bbox_kernel) -> min x, y, z, max x, y, z as floats in place, [6] = 1 when a finite point was seen
__global__ void cloud_bounds_result_kernel(unsigned* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool any = out[3] != 0u;
  for (int k = 0; k < 3; ++k) {
    const float lo = any ? dec(~out[k]) : 0.f, hi = any ? dec(out[3 + k]) : 0.f;
    out[k] = __float_as_uint(lo);
    out[3 + k] = __float_as_uint(hi);
  }
  out[6] = any ? 1u : 0u;
  out[7] = 0u;
}

struct StatLayout {
  size_t level1, row1, level2, row2, total;
};
inline StatLayout stat_layout(long m) {
  StatLayout L;
  const size_t lev = moment_scratch_bytes<kStatWords - 1>(m);
  L.level1 = 0;
  L.row1 = lev;
  L.level2 = L.row1 + 256;
  L.row2 = L.level2 + lev;
  L.total = L.row2 + 256;
  return L;
}

}  // namespace

extern "C" int atvs_cloud_knn_scratch_size(long n, long m, long* bytes) {
  return query_scratch_size(n, m, bytes);
}

extern "C" int atvs_cloud_knn(const void* grid, long grid_bytes, long n, const float* queries, long m, int k, int exclude_same_index,
                              void* scratch, long scratch_bytes, float* d2, int* idx, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints || k < 1 || k > kMaxK) return ATVS_ERR_SHAPE;
  if (exclude_same_index && m != n) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!grid || !queries || !scratch || !d2 || !idx) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const dim3 blocks((unsigned)cdiv(m, kThreads)), threads(kThreads);
  const int ex = exclude_same_index ? 1 : 0;
  return search(grid, grid_bytes, n, queries, m, scratch, scratch_bytes, st,
                [&](const GridHeader* hdr, const unsigned* S, const float4* rec, const unsigned* qS, const float4* qrec) {
                  if (k <= 4)
                    hipLaunchKernelGGL(cloud_knn_kernel<4>, blocks, threads, 0, st, hdr, S, rec, qS, qrec, m, k, ex, d2, idx);
                  else if (k <= 8)
                    hipLaunchKernelGGL(cloud_knn_kernel<8>, blocks, threads, 0, st, hdr, S, rec, qS, qrec, m, k, ex, d2, idx);
                  else if (k <= 16)
                    hipLaunchKernelGGL(cloud_knn_kernel<16>, blocks, threads, 0, st, hdr, S, rec, qS, qrec, m, k, ex, d2, idx);
                  else
                    hipLaunchKernelGGL(cloud_knn_kernel<32>, blocks, threads, 0, st, hdr, S, rec, qS, qrec, m, k, ex, d2, idx);
                });
}

extern "C" int atvs_cloud_radius_count(const void* grid, long grid_bytes, long n, const float* queries, long m, int exclude_same_index,
                                       void* scratch, long scratch_bytes, int* count, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (exclude_same_index && m != n) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!grid || !queries || !scratch || !count) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const int ex = exclude_same_index ? 1 : 0;
  return search(grid, grid_bytes, n, queries, m, scratch, scratch_bytes, st,
                [&](const GridHeader* hdr, const unsigned* S, const float4* rec, const unsigned* qS, const float4* qrec) {
                  hipLaunchKernelGGL(cloud_radius_count_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, st, hdr, S, rec, qS,
                                     qrec, m, ex, count);
                });
}

extern "C" int atvs_cloud_knn_mean(const float* d2, long m, int k, double* s, atvs_stream_t stream) {
  if (m < 0 || m > kMaxPoints || k < 1 || k > kMaxK) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!d2 || !s) return ATVS_ERR_NULL;
  hipLaunchKernelGGL(cloud_knn_mean_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, as_stream(stream), d2, m, k, s);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_cloud_sor_stats_scratch_size(long m, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)stat_layout(m).total;
  return ATVS_OK;
}

extern "C" int atvs_cloud_sor_stats(const double* s, long m, void* scratch, long scratch_bytes, void* out, atvs_stream_t stream) {
  if (m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!out || (m > 0 && (!s || !scratch))) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (m == 0) return hipMemsetAsync(out, 0, 3 * 8, st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  const StatLayout L = stat_layout(m);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  char* base = static_cast<char*>(scratch);
  unsigned long long* level1 = reinterpret_cast<unsigned long long*>(base + L.level1);
  unsigned long long* row1 = reinterpret_cast<unsigned long long*>(base + L.row1);
  unsigned long long* level2 = reinterpret_cast<unsigned long long*>(base + L.level2);
  unsigned long long* row2 = reinterpret_cast<unsigned long long*>(base + L.row2);
  const dim3 rows((unsigned)moment_rows(m)), threads(kThreads);
  hipLaunchKernelGGL(cloud_sor_sum_kernel, rows, threads, 0, st, s, m, moment_first(m, level1, row1));
  ATVS_LAUNCH_CHECK();
  int rc = moment_fold<kStatWords - 1>(m, level1, row1, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(cloud_sor_dev_kernel, rows, threads, 0, st, s, m, (const unsigned long long*)row1, moment_first(m, level2, row2));
  ATVS_LAUNCH_CHECK();
  rc = moment_fold<kStatWords - 1>(m, level2, row2, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(cloud_sor_result_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)row1, (const unsigned long long*)row2,
                     static_cast<unsigned long long*>(out));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_cloud_bounds(const float* points, long n, void* out, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!out || (n > 0 && !points)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  unsigned* box = static_cast<unsigned*>(out);
  if (hipMemsetAsync(box, 0, 8 * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n > 0) {
    hipLaunchKernelGGL(cloud_bbox_kernel, dim3(bbox_blocks(n)), dim3(kThreads), 0, st, points, n, box);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cloud_bounds_result_kernel, dim3(1), dim3(64), 0, st, box);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
