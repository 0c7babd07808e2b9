// Point-cloud scoring (gfx950): exact nearest neighbours within a radius between two clouds, and tolerance counts
// (ops/cloud.py, atvsnet/eval_cloud.py).
//
// THE DEFINITION (tests/cloud_restated.py restates it with numpy; the tests compare bit for bit).  Reference cloud P (n,3) float32,
// query cloud Q (m,3) float32, radius R > 0 (float32).  For a finite query q and a finite reference point p
//     dx = q.x - p.x,  dy = q.y - p.y,  dz = q.z - p.z          (float32)
//     d2 = (dx*dx + dy*dy) + dz*dz                              (float32, every operation rounded, no contraction: the library is
//                                                                built with -ffp-contract=off)
// Per query: d2min = the minimum of d2 over all finite reference points, idx = the LOWEST reference index attaining it; when
// (double)d2min > (double)R * (double)R, or the query is not finite, or no reference point is finite: d2min = +inf, idx = -1.
// Non-finite reference points are never neighbours.  The result is a function of P, Q, R alone: the grid below (cell size, origin,
// order of the points inside a cell, launch shape) cannot be seen in it.  A tolerance tau (double) counts a query when
// (double)d2min <= tau * tau (formed in double); tau > R is an argument error (distances beyond R are not known).
//
// THE GRID (cloud_grid.h: shared with cloud_knn.hip, as the walk over the 27 cells and the search's host side are).  A uniform grid
// of cubic cells of edge h over the bounding box of the finite reference points, built by counting sort:
//   bbox     per-wave minimum / maximum, then integer atomic max on order-preserving bit patterns (no float atomics anywhere);
//   params   one thread: origin = the box's minimum corner, h, cells per axis (all in double, kept in the grid's header);
//   count    cell of every point -> keys[i], one integer atomic add per point into the cell's counter;
//   scan     exclusive prefix sum of the counters (tiles of 2048, tile sums, add);
//   scatter  one returning integer atomic add per point on its cell's start: the point's slot; it is stored there as a 16-byte
//            record (x, y, z, original index), so a candidate is one global_load_dwordx4.  Afterwards counter c holds the END of
//            cell c = the start of cell c + 1; S = the counters with a zero in front: cell c is records S[c] .. S[c + 1].
// Non-finite points go to one extra bucket behind the last cell and are never read.  The grid is built once per reference cloud;
// memory is O(n + cells) with cells <= max(4096, min(8 n, 2^28)) known from n alone, so the host allocates before the box is known
// and the build never synchronises.
//
// THE QUERY.  The queries are sorted by the SAME cells with the same counting sort (queries further than one cell outside the grid,
// and non-finite ones, go to the extra bucket: not found).  One lane per query, in cell order: the lanes of a wavefront walk the same
// cells, their loads hit the same lines (identical addresses are one request).  x runs fastest in the cell index, so the 27 cells
// around a query are 9 contiguous runs of records.  Every lane keeps the minimum of (bits(d2) << 32) | index as one unsigned 64-bit
// integer: d2 >= +0, so its bit pattern orders as its value does (+inf above every finite one), and the low word is the tie rule.
// The results are written back to the queries' original positions.
//
// WHY 27 CELLS SUFFICE (the margin).  Let D be the true distance of a pair whose float32 d2 passes the test (double)d2 <= R^2.
// Each difference carries one rounding (relative 2^-24), squaring doubles it, the product and the two sums add one each: the
// float32 d2 is within 5 * 2^-24 < 2^-21 relative of D^2 (plus at most 3 * 2^-150 absolute where a product underflows), so
// D <= R (1 + 2^-21).  The cell edge is h >= max(R (1 + 2^-20), 2^-60): D / h <= (1 + 2^-21) / (1 + 2^-20) < 1 - 2^-22 (and where R is
// so small that underflow matters, h^2 = 2^-120 exceeds R^2 + 3 * 2^-150 by far).  A coordinate's cell is floor(((double)x - origin) /
// h) in double: at most 2^28 cells per axis and three roundings of 2^-53 put the computed quotient within 2^-23 of the exact one.
// Two points at most D apart on an axis therefore have computed quotients less than (1 - 2^-22) + 2 * 2^-23 = 1 apart, so their
// cells differ by at most one.  Clamping a query's cell into the grid never widens that difference (a clamp is monotone and
// 1-Lipschitz), and a query whose quotient lies below -1 or above the cell count is further than h (1 - 2^-23) > D from every
// reference point.  Where the box would need more cells than the cap (a sparse cloud with a small R), h is made larger, which the
// argument allows: a larger h only searches more.  With exactly h = R the argument fails, and so does the search: R = 0.25, query
// x = 0.25 - 2^-26 (cell 0), reference x = 0.5 (cell 2): dx rounds to 0.25, the float32 d2 is 0.0625 = R^2 exactly.
#include <math.h>

#include "common.h"
#include "cloud_grid.h"

namespace {

constexpr int kMaxTolerances = ATVS_CLOUD_MAX_TOLERANCES;

struct Tolerances {
  double t2[kMaxTolerances];
  int k;
};

__global__ void cloud_params_kernel(GridHeader* __restrict__ hdr, float radius, long cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  GridHeader g = *hdr;
  g.r2 = (double)radius * (double)radius;
  double h = fmax((double)radius * (1.0 + 0x1p-20), 0x1p-60);
  if (g.box[3] == 0u) {                                    // no finite reference point: one empty cell
    g.origin[0] = g.origin[1] = g.origin[2] = 0.0;
    g.dims[0] = g.dims[1] = g.dims[2] = 1;
  } else {
    float hi[3];
    for (int k = 0; k < 3; ++k) {
      g.origin[k] = (double)dec(~g.box[k]);
      hi[k] = dec(g.box[3 + k]);
    }
    double d[3];
    for (int it = 0;; ++it) {
      for (int k = 0; k < 3; ++k) d[k] = cell_coord(hi[k], g.origin[k], h) + 1.0;
      const double cells = d[0] * d[1] * d[2];
      if (cells <= (double)cap) break;
      if (it == 256) {                                     // cannot happen for finite boxes; one cell is always right
        h = 2.0 * fmax(fmax((double)hi[0] - g.origin[0], (double)hi[1] - g.origin[1]), (double)hi[2] - g.origin[2]);
        continue;
      }
      h *= 1.01 * fmax(cbrt(cells / (double)cap), 1.0);    // a coarser cell: invisible in the output (see the header comment)
    }
    for (int k = 0; k < 3; ++k) g.dims[k] = (int)d[k];
  }
  g.h = h;
  g.ncells = g.dims[0] * g.dims[1] * g.dims[2];
  *hdr = g;
}

__global__ __launch_bounds__(kThreads) void cloud_nearest_kernel(const GridHeader* __restrict__ hdr, const unsigned* __restrict__ S,
                                                                 const float4* __restrict__ rec, const unsigned* __restrict__ qS,
                                                                 const float4* __restrict__ qrec, long m, float* __restrict__ d2out,
                                                                 int* __restrict__ idxout) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const GridHeader g = *hdr;
  const float4 q = qrec[j];
  const int orig = __float_as_int(q.w);
  const unsigned long long none = (0x7f800000ull << 32) | 0xffffffffull;
  unsigned long long best = none;
  if (j < (long)qS[g.ncells]) {                             // not in the bucket of far / non-finite queries
    walk<4>(g, S, rec, q, [&](unsigned bits, unsigned i) {
      const unsigned long long key = ((unsigned long long)bits << 32) | i;
      best = key < best ? key : best;
    });
  }
  float d2 = __uint_as_float((unsigned)(best >> 32));
  int idx = (int)(unsigned)(best & 0xffffffffull);
  if (best == none || !((double)d2 <= g.r2)) {
    d2 = __uint_as_float(0x7f800000u);
    idx = -1;
  }
  d2out[orig] = d2;
  idxout[orig] = idx;
}

__global__ __launch_bounds__(kThreads) void cloud_counts_kernel(const float* __restrict__ d2, long m, Tolerances tol,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s[kMaxTolerances];
  if (threadIdx.x < kMaxTolerances) s[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned c[kMaxTolerances];
  for (int t = 0; t < kMaxTolerances; ++t) c[t] = 0u;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < m; i += (long)gridDim.x * kThreads) {
    const double v = (double)d2[i];
    for (int t = 0; t < kMaxTolerances; ++t) c[t] += (t < tol.k && v <= tol.t2[t]) ? 1u : 0u;
  }
  for (int t = 0; t < kMaxTolerances; ++t) {
    unsigned v = c[t];
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_down((int)v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s[t], (unsigned long long)v);
  }
  __syncthreads();
  if ((int)threadIdx.x < tol.k && s[threadIdx.x]) atomicAdd(counts + threadIdx.x, s[threadIdx.x]);
}

}  // namespace

extern "C" int atvs_cloud_grid_scratch_size(long n, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)layout_for(cell_cap(n), n, kHeaderBytes).total;
  return ATVS_OK;
}

extern "C" int atvs_cloud_grid_build(const float* points, long n, float radius, void* grid, long grid_bytes, atvs_stream_t stream) {
  if (!grid || (n > 0 && !points)) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!(radius > 0.f) || !(radius <= 3.4028234663852886e38f)) return ATVS_ERR_ARG;
  const long cap = cell_cap(n);
  const Layout L = layout_for(cap, n, kHeaderBytes);
  if (grid_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  GridHeader* hdr = static_cast<GridHeader*>(grid);
  if (hipMemsetAsync(grid, 0, kHeaderBytes, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n > 0) {
    hipLaunchKernelGGL(cloud_bbox_kernel, dim3(bbox_blocks(n)), dim3(kThreads), 0, st, points, n, hdr->box);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cloud_params_kernel, dim3(1), dim3(64), 0, st, hdr, radius, cap);
  ATVS_LAUNCH_CHECK();
  return counting_sort(points, n, hdr, static_cast<char*>(grid), L, cap, st);
}

extern "C" int atvs_cloud_nearest_scratch_size(long n, long m, long* bytes) {
  return query_scratch_size(n, m, bytes);
}

extern "C" int atvs_cloud_nearest(const void* grid, long grid_bytes, long n, const float* queries, long m, void* scratch,
                                  long scratch_bytes, float* d2, int* idx, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!grid || !queries || !scratch || !d2 || !idx) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  return search(grid, grid_bytes, n, queries, m, scratch, scratch_bytes, st,
                [&](const GridHeader* hdr, const unsigned* S, const float4* rec, const unsigned* qS, const float4* qrec) {
                  hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, st, hdr, S, rec, qS, qrec,
                                     m, d2, idx);
                });
}

extern "C" int atvs_cloud_counts(const float* d2, long m, const double* tolerances, int k, float radius, long long* counts,
                                 atvs_stream_t stream) {
  if (!counts || !tolerances || (m > 0 && !d2)) return ATVS_ERR_NULL;
  if (m < 0 || m > kMaxPoints || k < 1 || k > kMaxTolerances) return ATVS_ERR_SHAPE;
  if (!(radius > 0.f) || !(radius <= 3.4028234663852886e38f)) return ATVS_ERR_ARG;
  Tolerances tol;
  tol.k = k;
  for (int t = 0; t < kMaxTolerances; ++t) {
    const double tau = t < k ? tolerances[t] : 0.0;
    if (!(tau >= 0.0) || tau > (double)radius) return ATVS_ERR_ARG;
    tol.t2[t] = tau * tau;
  }
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(counts, 0, (size_t)kMaxTolerances * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (m == 0) return ATVS_OK;
  const unsigned blocks = (unsigned)(cdiv(m, kThreads * 8) < 2048 ? cdiv(m, kThreads * 8) : 2048);
  hipLaunchKernelGGL(cloud_counts_kernel, dim3(blocks), dim3(kThreads), 0, st, d2, m, tol, reinterpret_cast<unsigned long long*>(counts));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
