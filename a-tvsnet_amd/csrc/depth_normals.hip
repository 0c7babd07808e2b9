// Normals of a scene's depth maps, estimated from the maps themselves (gfx950): atvs_depth_normals_f32 fills the three normal
// floats of every pixel of the fusion slab (N, rows, cols, 4) = (nx, ny, nz, depth) in place, in one launch.
//
// A pixel's neighbours in its own depth map are its neighbours on the surface: no search, no eigen-solve.  Per pixel (x, y) of
// camera c with depth d, in float64 from the float32 inputs:
//   X(x, y, d) = M_inv (d x - p0, d y - p1, d - p2)                  (get3Dpoint_cu as fuse_pixel evaluates it)
//   neighbours R = (x + step, y), D = (x, y + step), L = (x - step, y), U = (x, y - step); one is valid when it lies inside the
//   image, its depth dn > 0 and |dn - d| <= depth_gate * d
//   for the quadrants (R,D), (D,L), (L,U), (U,R) in this order: both valid -> c = (Xa - X) x (Xb - X); |c| > 0 -> sum += c / |c|
//   |sum| = 0 (or d > 0 false) -> the normal is (0,0,0); else n = sum / |sum|, negated when n . (C - X) < 0: a visible surface
//   faces the camera that saw it, whatever the handedness of P.
// A zero normal gives acosf(0) = 90 degrees in fuse_pixel: under any threshold below 90 degrees a pixel without a usable
// neighbourhood agrees with nothing.
//
// The kernel reads only .w of the slab and writes only .xyz, so the slab is updated in place while neighbours are read.  One
// workgroup owns a run of 256 row-major pixels of one camera (fusion_grid.h, the count pass's layout): the camera is wave-uniform.
// Four neighbour loads of 4 bytes and ~150 FP64 operations per pixel; built with -ffp-contract=off like the other fusion sources.
#include "common.h"
#include "fusion_grid.h"

namespace {

struct D3 {
  double x, y, z;
};

__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ D3 back_project(const float* __restrict__ cam, int x, int y, double d) {
  const double ptx = d * (double)x - (double)cam[24], pty = d * (double)y - (double)cam[25], ptz = d - (double)cam[26];
  D3 X;
  X.x = (double)cam[12] * ptx + (double)cam[13] * pty + (double)cam[14] * ptz;
  X.y = (double)cam[15] * ptx + (double)cam[16] * pty + (double)cam[17] * ptz;
  X.z = (double)cam[18] * ptx + (double)cam[19] * pty + (double)cam[20] * ptz;
  return X;
}

// `slab` is read (.w) and written (.xyz) through this one pointer: no __restrict__
__global__ __launch_bounds__(kRun) void depth_normals_kernel(const float* __restrict__ cams, float* slab, int rows, int cols,
                                                             int runs_per_cam, int step, double gate) {
  const int b = blockIdx.x;
  const int view = b / runs_per_cam;                   // uniform over the workgroup
  const int p = (b - view * runs_per_cam) * kRun + (int)threadIdx.x;
  if (p >= rows * cols) return;
  const int y = p / cols, x = p - y * cols;
  const float* cam = cams + (size_t)view * 28;
  float* map = slab + (size_t)view * rows * cols * 4;
  const float df = map[(size_t)p * 4 + 3];
  D3 n = {0.0, 0.0, 0.0};
  if (df > 0.f) {
    const double d = (double)df;
    const D3 X = back_project(cam, x, y, d);
    // R, D, L, U; step >= 1 and x, y < 2^31 / step is not assumed: the sums are formed in long
    const long nx[4] = {(long)x + step, (long)x, (long)x - step, (long)x};
    const long ny[4] = {(long)y, (long)y + step, (long)y, (long)y - step};
    D3 e[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ok[k] = nx[k] >= 0 && nx[k] < cols && ny[k] >= 0 && ny[k] < rows;
      e[k] = {0.0, 0.0, 0.0};
      if (ok[k]) {
        const double dn = (double)map[((size_t)ny[k] * cols + (size_t)nx[k]) * 4 + 3];
        ok[k] = dn > 0.0 && fabs(dn - d) <= gate * d;
        if (ok[k]) e[k] = sub(back_project(cam, (int)nx[k], (int)ny[k], dn), X);
      }
    }
    D3 sum = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {                      // (R,D), (D,L), (L,U), (U,R)
      const int k2 = (k + 1) & 3;
      if (ok[k] && ok[k2]) {
        const D3 c = cross(e[k], e[k2]);
        const double len = sqrt(dot(c, c));
        if (len > 0.0) {
          sum.x += c.x / len;
          sum.y += c.y / len;
          sum.z += c.z / len;
        }
      }
    }
    const double len = sqrt(dot(sum, sum));
    if (len > 0.0) {
      n = {sum.x / len, sum.y / len, sum.z / len};
      const D3 C = {(double)cam[21], (double)cam[22], (double)cam[23]};
      if (dot(n, sub(C, X)) < 0.0) n = {-n.x, -n.y, -n.z};
    }
  }
  map[(size_t)p * 4 + 0] = (float)n.x;
  map[(size_t)p * 4 + 1] = (float)n.y;
  map[(size_t)p * 4 + 2] = (float)n.z;
}

}  // namespace

extern "C" int atvs_depth_normals_f32(const float* cams, float* normals_depths, int nviews, int rows, int cols, int step,
                                      float depth_gate, atvs_stream_t stream) {
  if (!cams || !normals_depths) return ATVS_ERR_NULL;
  int runs = 0;
  long blocks = 0;
  if (!scene_grid(nviews, rows, cols, &runs, &blocks)) return ATVS_ERR_SHAPE;
  if (step < 1 || !(depth_gate >= 0.f) || !(depth_gate <= 3.402823466e+38f)) return ATVS_ERR_ARG;      // negative, NaN, inf
  hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)blocks), dim3(kRun), 0, as_stream(stream), cams, normals_depths, rows,
                     cols, runs, step, (double)depth_gate);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
