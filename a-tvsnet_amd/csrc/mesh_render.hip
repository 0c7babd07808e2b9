// A triangle mesh rendered into the cameras of a scene (gfx950): nearest depth and face per pixel, and the occlusion pass that
// takes a rendered scan's pixels behind such a mesh out (atvsnet/eval_depth.py).  include/atvsnet_hip.h has the definition: the
// ray through a pixel centre against each face as three homogeneous edge functions in float64, every operation rounded
// (-ffp-contract=off), both windings, both sides of every edge inclusive, no near-plane clipping.  Per pixel the smallest 64-bit
// key (bits(z) << 32 | face) by an integer atomic min: the maps do not depend on the order in which the faces arrive.
//
// The result is a function of coverage alone, so a face may be tested against any SUPERSET of the pixels it covers (face_setup's
// box; DESIGN.md section 12.3a argues that it is one).  Two paths share face_setup and shade, so a (face, camera) pair has one box
// and a pixel one key whichever path reaches it:
//   face_kernel  one lane per face, the three vertices gathered once into registers as nine doubles; one workgroup per (kThreads
//                faces, kGroup cameras), laid out as scan_render.hip's splat_kernel.  The camera loop is wave-uniform and a camera's
//                16 doubles are scalar loads.  A pair whose box holds at most kSmallPixels pixels is rasterised by its lane; any
//                other is appended to the pair list with the number of kTile x kTile screen tiles of its box.
//   tile_kernel  the tile counts are scanned (cloud_scan.h), and a fixed grid of workgroups strides over the (pair, tile) items;
//                an item's pair is found by bisection in the scanned counts, its 4096 pixels go to the workgroup's lanes.  A
//                triangle that covers a whole image is spread over the CUs tile by tile.
// The pair list has a fixed capacity; the entry point walks the faces in chunks of capacity / n_cams, so a chunk cannot fill it:
// nothing is ever dropped, and nothing is read back by the host.  Both paths look at the pixel's key before the atomic and skip
// it when the pixel already holds a smaller one: an atomic executes at the memory side, the look hits in L2.
#include "common.h"
#include "scan_project.h"
#include "cloud_scan.h"

#include <math.h>

namespace {

constexpr int kGroup = 8;                                      // cameras per workgroup of face_kernel
constexpr int kSmallPixels = ATVS_MESH_RENDER_SMALL_PIXELS;    // the largest box a single lane walks
constexpr int kTile = 64;                                      // side of a screen tile of the large path
constexpr long kMaxPairs = 1L << 22;                           // capacity of the pair list (8 + 4 bytes each)
constexpr int kTileBlocks = 2048;                              // workgroups of tile_kernel: 8 per CU
constexpr unsigned long long kEmptyKey = ~0ull;

struct Face {
  double N0[3], N1[3], N2[3];   // B x D, D x A, A x B
  double det;
  int u0, u1, v0, v1;           // the box: pixels u0..u1 x v0..v1, inside the image and not empty
};

__device__ __forceinline__ void cross(const double* a, const double* b, double* n) {
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
}

// One face (P: its vertices, nine doubles) in one camera.  false: it takes part in no pixel of this camera.
__device__ __forceinline__ bool face_setup(const double* __restrict__ c, const double* P, int rows, int cols, double pixel_centre,
                                           Face* F) {
  double C[9];
  for (int i = 0; i < 3; ++i) {
    const double X = P[3 * i], Y = P[3 * i + 1], Z = P[3 * i + 2];
    for (int k = 0; k < 3; ++k) C[3 * i + k] = ((c[3 * k] * X + c[3 * k + 1] * Y) + c[3 * k + 2] * Z) + c[9 + k];
  }
  const double inf = (double)INFINITY;
  for (int i = 0; i < 9; ++i)
    if (!(fabs(C[i]) < inf)) return false;
  const double* A = C;
  const double* B = C + 3;
  const double* D = C + 6;
  if (!(A[2] > 0.0 || B[2] > 0.0 || D[2] > 0.0)) return false;
  // Two equal vertices: with A == B, A x B is exactly 0 and D x A exactly -(B x D), so E1 == -E0, E2 == 0 and S == 0 wherever
  // E0 == 0: no pixel is covered.  Decided here so that such a face (the TSDF extractor keeps them) never reaches the large path.
  if ((A[0] == B[0] && A[1] == B[1] && A[2] == B[2]) || (A[0] == D[0] && A[1] == D[1] && A[2] == D[2]) ||
      (B[0] == D[0] && B[1] == D[1] && B[2] == D[2]))
    return false;
  cross(B, D, F->N0);
  cross(D, A, F->N1);
  cross(A, B, F->N2);
  F->det = (A[0] * F->N0[0] + A[1] * F->N0[1]) + A[2] * F->N0[2];
  double bu0 = 0.0, bu1 = (double)(cols - 1), bv0 = 0.0, bv1 = (double)(rows - 1);          // the whole image
  if (A[2] > 0.0 && B[2] > 0.0 && D[2] > 0.0) {
    // Wholly in front: the projection is a triangle, and the pixels whose centres it holds lie in the box of its corners.  The
    // box is padded by a pixel; a face so thin that rounding could decide an edge function a pixel beyond it (doubled area under
    // 2^-40 fx fy times its extent in pixels) keeps the whole image.  u = x - pixel_centre is the pixel scale of the definition.
    const double x0 = ((A[0] / A[2]) * c[12] + c[14]) - pixel_centre, y0 = ((A[1] / A[2]) * c[13] + c[15]) - pixel_centre;
    const double x1 = ((B[0] / B[2]) * c[12] + c[14]) - pixel_centre, y1 = ((B[1] / B[2]) * c[13] + c[15]) - pixel_centre;
    const double x2 = ((D[0] / D[2]) * c[12] + c[14]) - pixel_centre, y2 = ((D[1] / D[2]) * c[13] + c[15]) - pixel_centre;
    const double xa = fmin(x0, fmin(x1, x2)), xb = fmax(x0, fmax(x1, x2));
    const double ya = fmin(y0, fmin(y1, y2)), yb = fmax(y0, fmax(y1, y2));
    const double area2 = fabs((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
    const double extent = fmax(1.0, fmax(xb - xa, yb - ya));
    const double thin = (0x1p-40 * fabs(c[12] * c[13])) * extent;
    if (fabs(xa) < inf && fabs(xb) < inf && fabs(ya) < inf && fabs(yb) < inf && area2 >= thin) {   // NaN fails: the whole image
      bu0 = fmax(bu0, ceil(xa) - 1.0);
      bu1 = fmin(bu1, floor(xb) + 1.0);
      bv0 = fmax(bv0, ceil(ya) - 1.0);
      bv1 = fmin(bv1, floor(yb) + 1.0);
      if (!(bu0 <= bu1 && bv0 <= bv1)) return false;                                          // beside the image
    }
  }
  F->u0 = (int)bu0;             // within 0..cols-1 and 0..rows-1: clamped in double before the conversion
  F->u1 = (int)bu1;
  F->v0 = (int)bv0;
  F->v1 = (int)bv1;
  return true;
}

// Pixel (u, v) of one camera's plane against one face.
__device__ __forceinline__ void shade(const Face& F, const double* __restrict__ c, int u, int v, double pixel_centre, int cols,
                                      unsigned long long* __restrict__ plane, unsigned face) {
  const double rx = (((double)u + pixel_centre) - c[14]) / c[12];
  const double ry = (((double)v + pixel_centre) - c[15]) / c[13];
  const double E0 = (F.N0[0] * rx + F.N0[1] * ry) + F.N0[2];
  const double E1 = (F.N1[0] * rx + F.N1[1] * ry) + F.N1[2];
  const double E2 = (F.N2[0] * rx + F.N2[1] * ry) + F.N2[2];
  const double S = (E0 + E1) + E2;
  const bool in = (E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0 && S > 0.0) || (E0 <= 0.0 && E1 <= 0.0 && E2 <= 0.0 && S < 0.0);
  if (!in) return;
  const double t = F.det / S;
  if (!(t > 0.0)) return;
  const float z = (float)t;
  if (!(z > 0.f && z < INFINITY)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)face;
  unsigned long long* p = plane + (size_t)v * cols + u;
  // The look: a stale value is never smaller than the current one (keys only fall), so a skip is always right.
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

__device__ __forceinline__ void gather(const float* __restrict__ verts, int i0, int i1, int i2, double* P) {
  const int idx[3] = {i0, i1, i2};
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) P[3 * i + k] = (double)verts[(size_t)idx[i] * 3 + k];
}

__device__ __forceinline__ long tiles_of(const Face& F) {
  return (long)((F.u1 - F.u0) / kTile + 1) * (long)((F.v1 - F.v0) / kTile + 1);
}

__global__ __launch_bounds__(kThreads) void face_kernel(const float* __restrict__ verts, long n_vertices, const int* __restrict__ faces,
                                                        long f_begin, long f_end, const double* __restrict__ cams, int n_cams, int rows,
                                                        int cols, double pixel_centre, unsigned long long* __restrict__ keys,
                                                        int2* __restrict__ pairs, unsigned* __restrict__ counts,
                                                        unsigned* __restrict__ n_pairs, unsigned capacity, int* __restrict__ error_out) {
  const long f = f_begin + (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= f_end) return;
  const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
    if (blockIdx.y == 0) atomicAdd(error_out, 1);             // once per face; F < 2^31
    return;
  }
  double P[9];
  gather(verts, i0, i1, i2, P);
  const int g0 = (int)blockIdx.y * kGroup;
  const int g1 = min(n_cams, g0 + kGroup);
  const size_t plane = (size_t)rows * (size_t)cols;
  for (int g = g0; g < g1; ++g) {                             // wave-uniform: c[] are uniform addresses
    const double* __restrict__ c = cams + (size_t)g * kCam;
    Face F;
    if (!face_setup(c, P, rows, cols, pixel_centre, &F)) continue;
    const long box = (long)(F.u1 - F.u0 + 1) * (long)(F.v1 - F.v0 + 1);
    if (box <= kSmallPixels) {
      unsigned long long* __restrict__ kp = keys + (size_t)g * plane;
      for (int v = F.v0; v <= F.v1; ++v)
        for (int u = F.u0; u <= F.u1; ++u) shade(F, c, u, v, pixel_centre, cols, kp, (unsigned)f);
    } else {
      const unsigned slot = atomicAdd(n_pairs, 1u);           // < capacity: a chunk has at most capacity pairs
      if (slot < capacity) {
        pairs[slot] = make_int2((int)f, g);
        counts[slot] = (unsigned)tiles_of(F);
      }
    }
  }
}

// scanned: capacity + 1 words, the exclusive scan of the tile counts (0 beyond the pairs appended), scanned[capacity] their sum.
__global__ __launch_bounds__(kThreads) void tile_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        const double* __restrict__ cams, int rows, int cols, double pixel_centre,
                                                        unsigned long long* __restrict__ keys, const int2* __restrict__ pairs,
                                                        const unsigned* __restrict__ scanned, unsigned capacity) {
  const unsigned total = scanned[capacity];
  const size_t plane = (size_t)rows * (size_t)cols;
  for (unsigned item = blockIdx.x; item < total; item += gridDim.x) {       // workgroup-uniform
    unsigned lo = 0u, hi = capacity;                          // the last pair with scanned[p] <= item: its count is not 0
    while (hi - lo > 1u) {
      const unsigned mid = lo + (hi - lo) / 2u;
      if (scanned[mid] <= item) lo = mid; else hi = mid;
    }
    const int2 pr = pairs[lo];
    const double* __restrict__ c = cams + (size_t)pr.y * kCam;
    double P[9];
    gather(verts, faces[(size_t)pr.x * 3], faces[(size_t)pr.x * 3 + 1], faces[(size_t)pr.x * 3 + 2], P);
    Face F;
    if (!face_setup(c, P, rows, cols, pixel_centre, &F)) continue;          // never: face_kernel listed the pair
    const int tile = (int)(item - scanned[lo]);
    const int tiles_x = (F.u1 - F.u0) / kTile + 1;
    const int ub = F.u0 + (tile % tiles_x) * kTile, vb = F.v0 + (tile / tiles_x) * kTile;
    unsigned long long* __restrict__ kp = keys + (size_t)pr.y * plane;
    for (int i = threadIdx.x; i < kTile * kTile; i += kThreads) {
      const int u = ub + (i % kTile), v = vb + (i / kTile);
      if (u <= F.u1 && v <= F.v1) shade(F, c, u, v, pixel_centre, cols, kp, (unsigned)pr.x);
    }
  }
}

__global__ __launch_bounds__(kThreads) void mesh_resolve_kernel(const unsigned long long* __restrict__ keys, long pixels,
                                                                float* __restrict__ depth, int* __restrict__ face) {
  const long i = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (i >= pixels) return;
  const unsigned long long k = keys[i];
  const bool empty = k == kEmptyKey;
  depth[i] = empty ? 0.f : __uint_as_float((unsigned)(k >> 32));
  face[i] = empty ? -1 : (int)(unsigned)(k & 0xffffffffull);
}

__global__ __launch_bounds__(kThreads) void occlude_kernel(const float* depth, const float* __restrict__ occluder, long pixels,
                                                           double tol, float* out) {        // depth may be out: no __restrict__
  const long i = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (i >= pixels) return;
  const float d = depth[i], o = occluder[i];
  const bool hidden = o > 0.f && d > 0.f && !((double)d <= (double)o * (1.0 + tol));
  out[i] = hidden ? 0.f : d;
}

// Pairs per chunk: within the list, and few enough that their tiles are counted in 32 bits.
inline long pair_capacity(int n_cams, int rows, int cols, long n_faces) {
  const long max_tiles = (long)cdiv(cols, kTile) * (long)cdiv(rows, kTile);
  long cap = kMaxPairs < 0xffffffffL / max_tiles ? kMaxPairs : 0xffffffffL / max_tiles;
  const long all = (n_faces > 0 ? n_faces : 1) * (long)n_cams;
  if (all < cap) cap = all;
  return cap > n_cams ? cap : n_cams;                         // one face in every camera at least; n_cams max_tiles < 2^32
}

struct Layout {
  size_t keys, pairs, counts, tiles, n_pairs, total;
  long capacity;
};

inline Layout layout(int n_cams, int rows, int cols, long n_faces) {
  Layout L;
  L.capacity = pair_capacity(n_cams, rows, cols, n_faces);
  L.keys = 0;
  L.pairs = align256((size_t)n_cams * (size_t)rows * (size_t)cols * sizeof(unsigned long long));
  L.counts = L.pairs + align256((size_t)L.capacity * sizeof(int2));
  L.tiles = L.counts + align256((size_t)(L.capacity + 1) * sizeof(unsigned));
  L.n_pairs = L.tiles + align256((size_t)scan_tiles(L.capacity + 1) * sizeof(unsigned));
  L.total = L.n_pairs + 256;
  return L;
}

}  // namespace

extern "C" int atvs_mesh_render_scratch_size(int n_cams, int rows, int cols, long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (check_maps(n_cams, rows, cols) != ATVS_OK || n_faces < 0 || n_faces >= (1L << 31)) return ATVS_ERR_SHAPE;
  *bytes = (long)layout(n_cams, rows, cols, n_faces).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_render(const float* vertices, long n_vertices, const int* faces, long n_faces, const double* cams, int n_cams,
                                int rows, int cols, double pixel_centre, void* scratch, long scratch_bytes, float* depth_out,
                                int* face_out, int* error_out, atvs_stream_t stream) {
  if (!cams || !scratch || !depth_out || !face_out || !error_out || (n_faces > 0 && (!faces || !vertices))) return ATVS_ERR_NULL;
  if (check_maps(n_cams, rows, cols) != ATVS_OK || n_vertices < 0 || n_vertices > kMaxPoints || n_faces < 0 || n_faces >= (1L << 31))
    return ATVS_ERR_SHAPE;
  const Layout L = layout(n_cams, rows, cols, n_faces);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  if (!(fabs(pixel_centre) < (double)INFINITY)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + L.keys);
  int2* pairs = reinterpret_cast<int2*>(base + L.pairs);
  unsigned* counts = reinterpret_cast<unsigned*>(base + L.counts);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  unsigned* n_pairs = reinterpret_cast<unsigned*>(base + L.n_pairs);
  const long pixels = (long)n_cams * rows * cols;
  if (hipMemsetAsync(keys, 0xFF, (size_t)pixels * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(error_out, 0, sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const long chunk = L.capacity / n_cams;                     // faces per chunk: chunk n_cams pairs at most
  for (long f0 = 0; f0 < n_faces; f0 += chunk) {
    const long f1 = f0 + chunk < n_faces ? f0 + chunk : n_faces;
    const long cap = (f1 - f0) * n_cams;                      // <= L.capacity
    if (hipMemsetAsync(counts, 0, (size_t)(cap + 1) * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    if (hipMemsetAsync(n_pairs, 0, sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    const dim3 grid((unsigned)cdiv(f1 - f0, kThreads), (unsigned)cdiv(n_cams, kGroup));
    hipLaunchKernelGGL(face_kernel, grid, dim3(kThreads), 0, st, vertices, n_vertices, faces, f0, f1, cams, n_cams, rows, cols,
                       pixel_centre, keys, pairs, counts, n_pairs, (unsigned)cap, error_out);
    ATVS_LAUNCH_CHECK();
    const int rc = exclusive_scan(counts, cap + 1, tiles, st);
    if (rc != ATVS_OK) return rc;
    hipLaunchKernelGGL(tile_kernel, dim3(kTileBlocks), dim3(kThreads), 0, st, vertices, faces, cams, rows, cols, pixel_centre, keys,
                       (const int2*)pairs, (const unsigned*)counts, (unsigned)cap);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)cdiv(pixels, kThreads)), dim3(kThreads), 0, st,
                     (const unsigned long long*)keys, pixels, depth_out, face_out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_depth_occlude(const float* depth, const float* occluder, long pixels, double tol, float* out,
                                  atvs_stream_t stream) {
  if (pixels < 0 || pixels >= (1L << 31)) return ATVS_ERR_SHAPE;
  if (pixels == 0) return ATVS_OK;
  if (!depth || !occluder || !out) return ATVS_ERR_NULL;
  if (!(tol >= 0.0 && tol < (double)INFINITY)) return ATVS_ERR_ARG;
  hipLaunchKernelGGL(occlude_kernel, dim3((unsigned)cdiv(pixels, kThreads)), dim3(kThreads), 0, as_stream(stream), depth, occluder,
                     pixels, tol, out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
