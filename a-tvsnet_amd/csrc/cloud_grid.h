// The uniform grid of the point-cloud searches, shared by cloud.hip (the nearest reference point) and cloud_knn.hip (the k nearest,
// the count inside the radius, the bounding box): the grid's header, the cell of a point, the buffers' layout, the bounding-box
// reduction, the counting sort that orders the reference points and the queries by cell, THE WALK over the 27 cells around a query
// (walk) and THE SEARCH every entry point launches through (search: the layout check, the queries' sort, the pointers).
// cloud.hip's header comment says what the grid is and why 27 cells suffice; nothing here can be seen in a result.
#pragma once
#include <math.h>

#include "common.h"
#include "cloud_scan.h"

namespace {

constexpr long kMinCells = 4096;
constexpr long kMaxCells = 1L << 28;
constexpr long kCellsPerPoint = 8;
constexpr size_t kHeaderBytes = 256;

struct GridHeader {                // the first kHeaderBytes of a grid
  double origin[3];                // minimum corner of the finite reference points
  double h;                        // cell edge
  double r2;                       // (double)R * (double)R
  int dims[3];                     // cells per axis, x fastest
  int ncells;                      // dims[0] * dims[1] * dims[2] <= cap; bucket `ncells` holds the points that are in no cell
  unsigned box[6];                 // bbox pass: ~enc(min x, y, z), enc(max x, y, z); 0 = no finite point seen
};
static_assert(sizeof(GridHeader) <= kHeaderBytes, "header");

inline long cell_cap(long n) { return n * kCellsPerPoint < kMinCells ? kMinCells : (n * kCellsPerPoint > kMaxCells ? kMaxCells : n * kCellsPerPoint); }

// One counting sort's buffers behind `front` bytes: S (cap + 2 counters), records (16 B per point), keys (4 B per point), tile sums.
struct Layout {
  size_t S, rec, keys, tiles, total;
};
inline Layout layout_for(long cap, long npts, size_t front) {
  Layout L;
  L.S = front;
  L.rec = L.S + align256((size_t)(cap + 2) * sizeof(unsigned));
  L.keys = L.rec + align256((size_t)npts * sizeof(float4));
  L.tiles = L.keys + align256((size_t)npts * sizeof(int));
  L.total = L.tiles + align256((size_t)scan_tiles(cap + 1) * sizeof(unsigned));
  return L;
}

// float bits <-> unsigned integers of the same order (finite values and infinities)
__device__ __forceinline__ unsigned enc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }

// The quotient the margin argument speaks of; ONE definition for the grid's size, the reference points and the queries.
__device__ __forceinline__ double cell_coord(float x, double origin, double h) { return floor(((double)x - origin) / h); }

// Cell index of a finite point, or `ncells` when it lies more than one cell outside the grid (queries only: a reference point is
// inside the box by construction).
__device__ __forceinline__ int cell_of(const GridHeader& g, float x, float y, float z, int* cx, int* cy, int* cz) {
  const double tx = cell_coord(x, g.origin[0], g.h), ty = cell_coord(y, g.origin[1], g.h), tz = cell_coord(z, g.origin[2], g.h);
  if (!(tx >= -1.0 && tx <= (double)g.dims[0] && ty >= -1.0 && ty <= (double)g.dims[1] && tz >= -1.0 && tz <= (double)g.dims[2]))
    return g.ncells;
  *cx = min(max((int)tx, 0), g.dims[0] - 1);
  *cy = min(max((int)ty, 0), g.dims[1] - 1);
  *cz = min(max((int)tz, 0), g.dims[2] - 1);
  return (*cz * g.dims[1] + *cy) * g.dims[0] + *cx;
}

// box[0..5] (zeroed by the caller) = ~enc(min x, y, z), enc(max x, y, z) over the finite points; 0 = no finite point seen
__global__ __launch_bounds__(kThreads) void cloud_bbox_kernel(const float* __restrict__ pts, long n, unsigned* __restrict__ box) {
  unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (!finite3(x, y, z)) continue;
    m[0] = max(m[0], ~enc(x)); m[1] = max(m[1], ~enc(y)); m[2] = max(m[2], ~enc(z));
    m[3] = max(m[3], enc(x));  m[4] = max(m[4], enc(y));  m[5] = max(m[5], enc(z));
  }
  for (int k = 0; k < 6; ++k) {
    unsigned v = m[k];
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(box + k, v);
  }
}
inline unsigned bbox_blocks(long n) { return (unsigned)(cdiv(n, kThreads) < 2048 ? cdiv(n, kThreads) : 2048); }

__global__ __launch_bounds__(kThreads) void cloud_count_kernel(const float* __restrict__ pts, long n, const GridHeader* __restrict__ hdr,
                                                               int* __restrict__ keys, unsigned* __restrict__ C) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const GridHeader g = *hdr;
  const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
  int cx, cy, cz;
  const int key = finite3(x, y, z) ? cell_of(g, x, y, z, &cx, &cy, &cz) : g.ncells;
  keys[i] = key;
  atomicAdd(C + key, 1u);
}

__global__ __launch_bounds__(kThreads) void cloud_scatter_kernel(const float* __restrict__ pts, long n, const int* __restrict__ keys,
                                                                 unsigned* __restrict__ C, float4* __restrict__ rec) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned pos = atomicAdd(C + keys[i], 1u);
  if (pos < (unsigned)n) rec[pos] = make_float4(pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], __int_as_float((int)i));
}

// count -> scan -> scatter of `npts` points by the cells of `hdr`, into the buffers of L inside `base`
inline int counting_sort(const float* pts, long npts, const GridHeader* hdr, char* base, const Layout& L, long cap, hipStream_t st) {
  unsigned* S = reinterpret_cast<unsigned*>(base + L.S);
  unsigned* C = S + 1;                                     // S[0] stays 0: cell c is records S[c] .. S[c + 1] after the scatter
  int* keys = reinterpret_cast<int*>(base + L.keys);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  float4* rec = reinterpret_cast<float4*>(base + L.rec);
  if (hipMemsetAsync(S, 0, (size_t)(cap + 2) * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (npts == 0) return ATVS_OK;
  const dim3 per_point((unsigned)cdiv(npts, kThreads));
  hipLaunchKernelGGL(cloud_count_kernel, per_point, dim3(kThreads), 0, st, pts, npts, hdr, keys, C);
  ATVS_LAUNCH_CHECK();
  const int rc = exclusive_scan(C, cap + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(cloud_scatter_kernel, per_point, dim3(kThreads), 0, st, pts, npts, (const int*)keys, C, rec);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

// What atvs_cloud_nearest_scratch_size and atvs_cloud_knn_scratch_size report: the queries' sort.
inline int query_scratch_size(long n, long m, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)layout_for(cell_cap(n), m, 0).total;
  return ATVS_OK;
}

// Calls visit(d2 bits, reference index) for every finite reference point in the 27 cells around the sorted query q, 9 contiguous
// runs of records; Unroll: of the loop over a run.  S and rec are the kernels' own __restrict__ parameters: not said again here.
template <int Unroll, class Visit>
__device__ __forceinline__ void walk(const GridHeader& g, const unsigned* S, const float4* rec, const float4& q, Visit visit) {
  int cx, cy, cz;
  cell_of(g, q.x, q.y, q.z, &cx, &cy, &cz);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dims[0] - 1);
  for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dims[2] - 1); ++z) {
    for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dims[1] - 1); ++y) {
      const int row = (z * g.dims[1] + y) * g.dims[0];
      const unsigned b = S[row + x0], e = S[row + x1 + 1];
#pragma unroll Unroll
      for (unsigned p = b; p < e; ++p) {
        const float4 r = rec[p];
        const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        visit(__float_as_uint(d2), (unsigned)__float_as_int(r.w));
      }
    }
  }
}

// The query side of a search, the same for every kernel that walks the grid: the layouts of the grid and of the queries' sort
// inside the caller's buffers, checked against their sizes; the queries' counting sort; then `launch(hdr, S, rec, qS, qrec)`.
template <class Launch>
int search(const void* grid, long grid_bytes, long n, const float* queries, long m, void* scratch, long scratch_bytes, hipStream_t st,
           Launch launch) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  const long cap = cell_cap(n);
  const Layout G = layout_for(cap, n, kHeaderBytes), Q = layout_for(cap, m, 0);
  if (grid_bytes < (long)G.total || scratch_bytes < (long)Q.total) return ATVS_ERR_SHAPE;
  const char* g = static_cast<const char*>(grid);
  const GridHeader* hdr = reinterpret_cast<const GridHeader*>(g);
  char* q = static_cast<char*>(scratch);
  const int rc = counting_sort(queries, m, hdr, q, Q, cap, st);
  if (rc != ATVS_OK) return rc;
  launch(hdr, reinterpret_cast<const unsigned*>(g + G.S), reinterpret_cast<const float4*>(g + G.rec),
         reinterpret_cast<const unsigned*>(q + Q.S), reinterpret_cast<const float4*>(q + Q.rec));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

}  // namespace
