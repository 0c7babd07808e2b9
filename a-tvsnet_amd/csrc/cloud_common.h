// The point-cloud family's constants and one-line helpers, ONE definition each: the grid / scan / tree / register side takes them
// through cloud_scan.h, the renderer and the visibility query through scan_project.h.
#pragma once
#include <math.h>

#include "common.h"

namespace {
constexpr int kThreads = 256;                          // lanes per workgroup: one per point, query, slot or pixel
constexpr long kMaxPoints = 1L << 30;                  // rows of a cloud
__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float big = __uint_as_float(0x7f800000u);
  return fabsf(x) < big && fabsf(y) < big && fabsf(z) < big;        // NaN fails every comparison
}
}  // namespace
