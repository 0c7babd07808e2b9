// Scanner free space (gfx950): how far a point lies in front of or behind what a laser scanner saw along the point's ray -- the
// visibility half of the ETH3D-style score of atvsnet/eval_cloud.py (the definition is in
// include/atvsnet_hip.h, restated in tests/cloud_eth3d_restated.py).
//
// A scanner's view of its own scan is a cube map: six 90-degree pinhole cameras at its origin, rendered by atvs_scan_render as
// they stand.  atvs_cloud_scan_excess looks a point up in them through scan_project.h -- the renderer's own projection, so a scan
// point and a query on one ray reach one pixel -- takes the nearest non-empty depth of a (2 w + 1)^2 window inside that face and
// returns the signed distance along the ray, r (1 - z_scan / c_2): negative in front of the scan (free space), positive behind it.
//   one lane per point, the point held in registers as three doubles.  The scanner and face loops are wave-uniform: a lane that has
//   found its face skips the rest under the execution mask, and a camera's 16 doubles come from addresses every lane shares.  The
//   window is (2 w + 1)^2 plain 4-byte gathers from the maps.  No atomics, no LDS, no host synchronisation: the output is a
//   function of the inputs alone.
// What bounds it.  Per (point, scanner): up to six projections of ~40 float64 operations with two divisions each (the first face
// in view ends them: 3.5 on average), then one square root, one more division and (2 w + 1)^2 gathers.  The maps of a scene (a
// few scanners of 6 x 1024^2 floats: 25 MB each) stay in the L2 / Infinity Cache; neighbouring points look at neighbouring pixels
// only where the cloud is ordered in space.  The float64 arithmetic is the larger part at every w this takes.
#include "common.h"
#include "scan_project.h"

#include <math.h>

namespace {

constexpr int kFaces = 6;
constexpr int kMaxWindow = ATVS_CLOUD_SCAN_MAX_WINDOW;

__global__ __launch_bounds__(kThreads) void scan_excess_kernel(const float* __restrict__ pts, long m, const double* __restrict__ cams,
                                                               const float* __restrict__ maps, int n_scanners, int size,
                                                               double pixel_centre, int window, float* __restrict__ excess,
                                                               int* __restrict__ scanner) {
  const long p = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (p >= m) return;
  const float xf = pts[p * 3 + 0], yf = pts[p * 3 + 1], zf = pts[p * 3 + 2];
  const float big = __uint_as_float(0x7f800000u);
  const bool finite = finite3(xf, yf, zf);
  const double X = (double)xf, Y = (double)yf, Z = (double)zf;
  const double hi = (double)size;
  const size_t plane = (size_t)size * (size_t)size;
  double best = (double)INFINITY;
  int best_s = -1;
  for (int s = 0; s < n_scanners; ++s) {                      // wave-uniform, as the face loop is
    ScanProjection P;
    int face = -1;
    for (int f = 0; f < kFaces; ++f) {
      if (face >= 0 || !finite) continue;                     // the first face in view: the tie rule on cube edges
      ScanProjection Q;
      if (scan_project(cams + (size_t)(s * kFaces + f) * kCam, X, Y, Z, pixel_centre, 0.0, hi, hi, &Q)) {
        P = Q;
        face = f;
      }
    }
    if (face < 0) continue;                                   // no face in view (the scanner's own origin is such a point)
    const int u = (int)floor(P.xs), v = (int)floor(P.ys);     // within [0, size) x [0, size)
    const float* __restrict__ map = maps + (size_t)(s * kFaces + face) * plane;
    const int v0 = max(v - window, 0), v1 = min(v + window, size - 1);      // windows do not cross cube edges
    const int u0 = max(u - window, 0), u1 = min(u + window, size - 1);
    float z_scan = big;
    for (int vv = v0; vv <= v1; ++vv)
      for (int uu = u0; uu <= u1; ++uu) {
        const float d = map[(size_t)vv * size + uu];
        if (d != 0.f && d < z_scan) z_scan = d;
      }
    if (!(z_scan < big)) continue;                            // the whole window is empty: this scanner does not observe the point
    const double r = sqrt((P.c0 * P.c0 + P.c1 * P.c1) + P.c2 * P.c2);
    const double e = r * (1.0 - (double)z_scan / P.c2);
    if (e < best) {                                           // strict: the lowest scanner attaining the minimum
      best = e;
      best_s = s;
    }
  }
  excess[p] = best_s >= 0 ? (float)best : big;
  scanner[p] = best_s;
}

}  // namespace

extern "C" int atvs_cloud_scan_excess(const float* points, long m, const double* cams, const float* maps, int n_scanners, int size,
                                      double pixel_centre, int window, float* excess, int* scanner, atvs_stream_t stream) {
  if (m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (n_scanners < 1 || n_scanners > kMaxCams / kFaces) return ATVS_ERR_SHAPE;              // before the product below can overflow
  if (check_maps(n_scanners * kFaces, size, size) != ATVS_OK) return ATVS_ERR_SHAPE;
  if (!cams || !maps || (m > 0 && (!points || !excess || !scanner))) return ATVS_ERR_NULL;
  if (window < 0 || window > kMaxWindow) return ATVS_ERR_ARG;
  if (!(fabs(pixel_centre) < (double)INFINITY)) return ATVS_ERR_ARG;
  if (m == 0) return ATVS_OK;
  hipLaunchKernelGGL(scan_excess_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, as_stream(stream), points, m, cams, maps,
                     n_scanners, size, pixel_centre, window, excess, scanner);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
