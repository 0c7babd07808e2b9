// The exclusive prefix sum of unsigned counters shared by the point-cloud kernels: exclusive_scan(), called by cloud_grid.h's
// counting_sort (the cell starts) and cloud_register.hip's atvs_cloud_voxel_downsample (the output positions).  Three launches: tiles
// of kScanTile counters scanned in place, the tile sums scanned by one workgroup, the sums added back.  Integer arithmetic only: exact
// in any launch shape.  cloud_grid.h, cloud_tree.h and cloud_register.hip take cloud_common.h's constants through this file.
#pragma once
#include "common.h"
#include "cloud_common.h"

namespace {

constexpr int kScanItems = 8;                          // counters per thread of a scan tile
constexpr int kScanTile = kThreads * kScanItems;       // 2048

__device__ __forceinline__ unsigned wave_inclusive(unsigned v, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned y = (unsigned)__shfl_up((int)v, off);
    if (lane >= off) v += y;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void cloud_scan_tile_kernel(unsigned* __restrict__ a, long count, unsigned* __restrict__ tile_sum) {
  __shared__ unsigned wsum[kThreads / 64];
  const long base = (long)blockIdx.x * kScanTile + (long)threadIdx.x * kScanItems;
  unsigned v[kScanItems], run = 0u;
  for (int k = 0; k < kScanItems; ++k) {
    const unsigned t = base + k < count ? a[base + k] : 0u;
    v[k] = run;
    run += t;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned incl = wave_inclusive(run, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned before = 0u, total = 0u;
  for (int k = 0; k < kThreads / 64; ++k) {
    if (k < w) before += wsum[k];
    total += wsum[k];
  }
  const unsigned excl = before + incl - run;
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < count) a[base + k] = v[k] + excl;
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void cloud_scan_sums_kernel(unsigned* __restrict__ tile_sum, long tiles) {
  __shared__ unsigned wsum[16];
  __shared__ unsigned carry;
  if (threadIdx.x == 0) carry = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long b = 0; b < tiles; b += 1024) {
    const long i = b + threadIdx.x;
    const unsigned t = i < tiles ? tile_sum[i] : 0u;
    const unsigned incl = wave_inclusive(t, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned before = 0u, total = 0u;
    for (int k = 0; k < 16; ++k) {
      if (k < w) before += wsum[k];
      total += wsum[k];
    }
    if (i < tiles) tile_sum[i] = carry + before + incl - t;
    __syncthreads();
    if (threadIdx.x == 0) carry += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void cloud_scan_add_kernel(unsigned* __restrict__ a, long count, const unsigned* __restrict__ tile_sum) {
  const unsigned add = tile_sum[blockIdx.x];
  const long base = (long)blockIdx.x * kScanTile;
  for (int k = 0; k < kScanItems; ++k) {
    const long i = base + (long)k * kThreads + threadIdx.x;
    if (i < count) a[i] += add;
  }
}

inline long scan_tiles(long count) { return (count + kScanTile - 1) / kScanTile; }     // the words of a caller's `tiles` buffer

// Exclusive scan of `count` counters in place: tiles of kScanTile, the tile sums by one workgroup, then added back.
inline int exclusive_scan(unsigned* counters, long count, unsigned* tiles, hipStream_t st) {
  const long nt = scan_tiles(count);
  hipLaunchKernelGGL(cloud_scan_tile_kernel, dim3((unsigned)nt), dim3(kThreads), 0, st, counters, count, tiles);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_scan_sums_kernel, dim3(1), dim3(1024), 0, st, tiles, nt);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_scan_add_kernel, dim3((unsigned)nt), dim3(kThreads), 0, st, counters, count, (const unsigned*)tiles);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

}  // namespace
