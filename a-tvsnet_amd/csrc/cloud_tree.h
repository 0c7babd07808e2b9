// The fixed-shape sum of the point-cloud kernels (cloud_register.hip: the 18 pair moments and the 37 point-to-plane moments;
// cloud_knn.hip: the two passes of the outlier statistics).  A row is one int64 count and N doubles.  Term i belongs to workgroup i / (256 L), thread (i mod 256),
// L = ATVS_CLOUD_MOMENT_RUN: a thread adds its at most L terms i, i + 256, ... in that order into accumulators that start at +0,
// the 64 lanes of a wavefront fold in six steps (lane j takes lane j + 32, then + 16, ... + 1), the four wavefronts as
// (w0 + w1) + (w2 + w3): one row per workgroup.  Rows are folded 256 at a time by the same tree (rows beyond the end are +0) until
// one is left.  No atomics: the same input gives the same words bit for bit.  cloud_register.hip's header comment counts the
// rounding additions an accumulator can see: no more than L + ceil(log2 m).
#pragma once
#include "common.h"
#include "cloud_scan.h"

namespace {

constexpr int kMomentRun = ATVS_CLOUD_MOMENT_RUN;      // L: serial additions per accumulator before the tree
constexpr long kMomentTile = (long)kThreads * kMomentRun;

template <int N>
struct MomentShared {
  long long cnt[kThreads / 64];
  double sum[kThreads / 64][N];
};

// The fixed tree of one workgroup: cnt is the count, v[0..N-1] the sums.  The result is valid in thread 0.
template <int N>
__device__ __forceinline__ void block_tree(long long& cnt, double* v, MomentShared<N>& sh) {
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] + __shfl_down(v[k], off);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sh.cnt[w] = cnt;
#pragma unroll
    for (int k = 0; k < N; ++k) sh.sum[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt = (sh.cnt[0] + sh.cnt[1]) + (sh.cnt[2] + sh.cnt[3]);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (sh.sum[0][k] + sh.sum[1][k]) + (sh.sum[2][k] + sh.sum[3][k]);
  }
}

template <int N>
__device__ __forceinline__ void store_row(unsigned long long* row, long long cnt, const double* v) {
  row[0] = (unsigned long long)cnt;
#pragma unroll
  for (int k = 0; k < N; ++k) row[1 + k] = (unsigned long long)__double_as_longlong(v[k]);
}

// The row of this workgroup: term(i, cnt, v) adds term i (or nothing) to the thread's accumulators.
template <int N, class Term>
__device__ __forceinline__ void moment_row(long m, Term term, unsigned long long* __restrict__ rows, MomentShared<N>& sh) {
  long long cnt = 0;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  const long base = (long)blockIdx.x * kMomentTile + threadIdx.x;
  for (int r = 0; r < kMomentRun; ++r) {
    const long i = base + (long)r * kThreads;
    if (i >= m) break;
    term(i, cnt, v);
  }
  block_tree<N>(cnt, v, sh);
  if (threadIdx.x == 0) store_row<N>(rows + (long)blockIdx.x * (N + 1), cnt, v);
}

// 256 rows -> one, by the same tree; rows beyond `count` are +0
template <int N>
__global__ __launch_bounds__(kThreads) void cloud_moments_fold_kernel(const unsigned long long* __restrict__ in, long count,
                                                                      unsigned long long* __restrict__ out) {
  __shared__ MomentShared<N> sh;
  const long r = (long)blockIdx.x * kThreads + threadIdx.x;
  long long cnt = 0;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  if (r < count) {
    cnt = (long long)in[r * (N + 1)];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = __longlong_as_double((long long)in[r * (N + 1) + 1 + k]);
  }
  block_tree<N>(cnt, v, sh);
  if (threadIdx.x == 0) store_row<N>(out + (long)blockIdx.x * (N + 1), cnt, v);
}

inline long moment_rows(long m) { return (m + kMomentTile - 1) / kMomentTile; }

// Bytes of the levels between the first rows and the last one (none when one workgroup covers m).
template <int N>
inline size_t moment_scratch_bytes(long m) {
  long rows = 0;
  for (long r = moment_rows(m); r > 1; r = (r + kThreads - 1) / kThreads) rows += r;
  return (((size_t)(rows + 1) * (N + 1) * 8) + 255) & ~(size_t)255;
}

// Where the first launch writes its moment_rows(m) rows: `res` itself when that is one row, else `level`.
inline unsigned long long* moment_first(long m, unsigned long long* level, unsigned long long* res) { return moment_rows(m) == 1 ? res : level; }

// Folds the moment_rows(m) rows in `level` down to one in `res`.
template <int N>
inline int moment_fold(long m, unsigned long long* level, unsigned long long* res, hipStream_t st) {
  long rows = moment_rows(m);
  while (rows > 1) {
    const long next = (rows + kThreads - 1) / kThreads;
    unsigned long long* to = next == 1 ? res : level + rows * (N + 1);
    hipLaunchKernelGGL(cloud_moments_fold_kernel<N>, dim3((unsigned)next), dim3(kThreads), 0, st, (const unsigned long long*)level, rows, to);
    ATVS_LAUNCH_CHECK();
    level = to;
    rows = next;
  }
  return ATVS_OK;
}

}  // namespace
