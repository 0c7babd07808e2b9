// The projection of a point into one camera of atvs_scan_render's layout, shared by the renderer (scan_render.hip: where a scan
// point lands) and the visibility query (cloud_visibility.hip: which pixel a reconstruction point looks at).  ONE definition: a scan
// point and a query on the same ray reach the same pixel.  Float64, every operation rounded (-ffp-contract=off), in the order of
// include/atvsnet_hip.h.  With it what both say of a set of cameras: a camera's length, their number's limit, the maps' shape check.
#pragma once
#include "common.h"
#include "cloud_common.h"

#include <math.h>

constexpr int kCam = 16;               // R (3x3 row-major), t (3), fx, fy, cx, cy
constexpr int kMaxCams = ATVS_SCAN_RENDER_MAX_CAMS;

static inline int check_maps(int n_cams, int rows, int cols) {        // n_cams maps of rows x cols: pixels are indexed in 31 bits
  if (n_cams <= 0 || rows <= 0 || cols <= 0 || n_cams > kMaxCams) return ATVS_ERR_SHAPE;
  return (double)n_cams * (double)rows * (double)cols >= 2147483648.0 ? ATVS_ERR_SHAPE : ATVS_OK;
}

struct ScanProjection {
  double c0, c1, c2;      // the point in the camera's frame
  double xs, ys;          // pixel coordinates shifted so that floor() is the pixel
  float z;                // (float)c2
};

// cam: R (3x3 row-major), t (3), fx, fy, cx, cy.  The pair takes part when c2 > 0, z is finite and > 0, and
// lo <= xs < hx, lo <= ys < hy (lo = -splat, hx = cols + splat, hy = rows + splat), compared in double before any integer
// conversion: a point that projects 1e30 pixels away (or to NaN) never reaches the cast.  false: *P is partly written.
__device__ __forceinline__ bool scan_project(const double* __restrict__ c, double X, double Y, double Z, double pixel_centre, double lo,
                                             double hx, double hy, ScanProjection* P) {
  const double c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11];
  if (!(c2 > 0.0)) return false;                              // behind the camera, on its plane, or NaN
  const float z = (float)c2;
  if (!(z > 0.f && z < INFINITY)) return false;               // beyond float32's range either way
  const double c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9];
  const double c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10];
  const double x = (c0 / c2) * c[12] + c[14];
  const double y = (c1 / c2) * c[13] + c[15];
  const double xs = (x - pixel_centre) + 0.5;
  const double ys = (y - pixel_centre) + 0.5;
  if (!(xs >= lo && xs < hx && ys >= lo && ys < hy)) return false;
  P->c0 = c0;
  P->c1 = c1;
  P->c2 = c2;
  P->xs = xs;
  P->ys = ys;
  P->z = z;
  return true;
}
