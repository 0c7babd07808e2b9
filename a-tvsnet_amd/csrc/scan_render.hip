// A scan rendered into the cameras of a scene (gfx950): the ground-truth depth maps of atvsnet/eval_depth.py.
//
// atvs_scan_render projects every scan point into every camera in float64 (the projection of colmap.hip's depth-range kernel, in
// the same order) and keeps, per pixel, the nearest depth as a float32.  A positive float32 orders as its bit pattern does, so the
// minimum is an integer atomic min on `unsigned`: the planes do not depend on the order in which the points arrive.  No float
// atomics, no 64-bit keys, no host synchronisation.
//   splat    one lane per point, the point held in registers as three doubles; one workgroup per (kThreads points, kGroup
//            cameras), the grid laid out as colmap.hip's histogram pass (x: point tiles, y: camera groups).  The camera loop is
//            wave-uniform and a camera's 16 doubles are read from addresses every lane shares (scalar loads).  Two planes per
//            camera, both all-ones at first (hipMemsetAsync 0xFF): `near` takes the point's own pixel, `front` every pixel of
//            the (2 splat + 1)^2 window around it that lies inside the image.
//   resolve  one lane per pixel: 0 where nothing landed; the nearest depth where it is no further than the window's nearest
//            depth times (1 + occlusion_tol); else 0 (a background point seen through a hole of a nearer surface).
// With splat = 0 the window is the pixel itself, front == near and every near pixel survives: the front plane is then neither
// written nor read (half the atomics, the same output).
//
// What bounds it.  Per (camera, point) pair: 9 multiplications and 9 additions for c, two float64 divisions (each a dozen
// float64 instructions: scale, reciprocal estimate, Newton steps, fix-up), the two affine maps, two floors and eight compares --
// about 40 float64 operations plus the divisions -- and then (2 splat + 1)^2 + 1 atomics of 4 bytes, each its own memory
// transaction unless neighbouring lanes hit one 64-byte line.  The planes of a scene (50 cameras of 228 x 120: 11 MB) stay in
// the L2 / Infinity Cache; the points are read once per camera group (12 bytes per kGroup pairs).  At splat = 0 the float64
// arithmetic is the larger part; from splat = 2 (26 atomics per pair in view) the atomics are.  DESIGN.md section 12.3.
#include "common.h"
#include "scan_project.h"

#include <math.h>

namespace {

constexpr int kGroup = 8;              // cameras per workgroup (of kThreads points, one lane per point)
constexpr int kMaxSplat = ATVS_SCAN_RENDER_MAX_SPLAT;
constexpr unsigned kEmpty = 0xffffffffu;

__host__ __device__ inline size_t plane_bytes(int n_cams, int rows, int cols) {
  return (size_t)n_cams * (size_t)rows * (size_t)cols * sizeof(unsigned);
}

__global__ __launch_bounds__(kThreads) void splat_kernel(const float* __restrict__ pts, long n, const double* __restrict__ cams,
                                                         int n_cams, int rows, int cols, double pixel_centre, int splat,
                                                         unsigned* __restrict__ near, unsigned* __restrict__ front) {
  const long p = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (p >= n) return;
  const double X = (double)pts[p * 3 + 0], Y = (double)pts[p * 3 + 1], Z = (double)pts[p * 3 + 2];
  const int g0 = (int)blockIdx.y * kGroup;
  const int g1 = min(n_cams, g0 + kGroup);
  const double lo = -(double)splat;
  const double hx = (double)cols + (double)splat, hy = (double)rows + (double)splat;
  const size_t plane = (size_t)rows * (size_t)cols;
  for (int g = g0; g < g1; ++g) {                             // wave-uniform: c[] are uniform addresses
    ScanProjection P;                                         // scan_project.h: shared with the visibility query
    if (!scan_project(cams + (size_t)g * kCam, X, Y, Z, pixel_centre, lo, hx, hy, &P)) continue;
    const int u = (int)floor(P.xs), v = (int)floor(P.ys);     // within [-splat, cols + splat) x [-splat, rows + splat)
    const unsigned bits = __float_as_uint(P.z);
    if (u >= 0 && u < cols && v >= 0 && v < rows) atomicMin(near + (size_t)g * plane + (size_t)v * cols + u, bits);
    if (splat == 0) continue;
    unsigned* __restrict__ fg = front + (size_t)g * plane;
    const int v0 = max(v - splat, 0), v1 = min(v + splat, rows - 1);
    const int u0 = max(u - splat, 0), u1 = min(u + splat, cols - 1);
    for (int vv = v0; vv <= v1; ++vv)
      for (int uu = u0; uu <= u1; ++uu) atomicMin(fg + (size_t)vv * cols + uu, bits);
  }
}

__global__ __launch_bounds__(kThreads) void resolve_kernel(const unsigned* __restrict__ near, const unsigned* __restrict__ front,
                                                           long pixels, int splat, double occlusion_tol,
                                                           float* __restrict__ depth) {
  const long i = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (i >= pixels) return;
  const unsigned nb = near[i];
  float d = 0.f;
  if (nb != kEmpty) {
    const float z = __uint_as_float(nb);
    d = z;
    if (splat > 0) {                                          // a near pixel lies in its own window: front[i] <= nb
      const float zf = __uint_as_float(front[i]);
      if (!((double)z <= (double)zf * (1.0 + occlusion_tol))) d = 0.f;
    }
  }
  depth[i] = d;
}

}  // namespace

extern "C" int atvs_scan_render_scratch_size(int n_cams, int rows, int cols, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (check_maps(n_cams, rows, cols) != ATVS_OK) return ATVS_ERR_SHAPE;
  *bytes = (long)(2 * plane_bytes(n_cams, rows, cols));
  return ATVS_OK;
}

extern "C" int atvs_scan_render(const float* points, long n, const double* cams, int n_cams, int rows, int cols,
                                double pixel_centre, int splat, double occlusion_tol, void* scratch, long scratch_bytes,
                                float* depth_out, atvs_stream_t stream) {
  if (!cams || !scratch || !depth_out || (n > 0 && !points)) return ATVS_ERR_NULL;
  if (check_maps(n_cams, rows, cols) != ATVS_OK || n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  const size_t pb = plane_bytes(n_cams, rows, cols);
  if (scratch_bytes < (long)(2 * pb)) return ATVS_ERR_SHAPE;
  if (splat < 0 || splat > kMaxSplat) return ATVS_ERR_ARG;
  if (!(occlusion_tol >= 0.0 && occlusion_tol < (double)INFINITY)) return ATVS_ERR_ARG;
  if (!(fabs(pixel_centre) < (double)INFINITY)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  unsigned* near = static_cast<unsigned*>(scratch);
  unsigned* front = reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + pb);
  if (hipMemsetAsync(scratch, 0xFF, splat > 0 ? 2 * pb : pb, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n > 0) {
    const dim3 grid((unsigned)cdiv(n, kThreads), (unsigned)cdiv(n_cams, kGroup));
    hipLaunchKernelGGL(splat_kernel, grid, dim3(kThreads), 0, st, points, n, cams, n_cams, rows, cols, pixel_centre, splat, near,
                       front);
    ATVS_LAUNCH_CHECK();
  }
  const long pixels = (long)n_cams * rows * cols;
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)cdiv(pixels, kThreads)), dim3(kThreads), 0, st, near, front, pixels, splat,
                     occlusion_tol, depth_out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
