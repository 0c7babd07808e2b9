// Undistortion of COLMAP's distorted camera models (gfx950): the per-camera sampling map and the image gather of
// atvsnet/undistort.py, what `colmap image_undistorter` does to the images, restated.
//
// atvs_undistort_map   one thread per pixel of the undistorted camera: the pixel's ray through the model's forward distortion, in
//                      float64 in the operation order of the numpy restatement (the library is built with -ffp-contract=off; only
//                      atan, in the fisheye models, is not pinned to the last bit), the source coordinate stored as 22.10 fixed
//                      point.  The model is a template parameter: uniform over the launch.
// atvs_undistort_remap a pure gather in integers, prepare.hip's kind of arithmetic: four consecutive output pixels per thread (two
//                      16-byte loads of the map, three dword stores), taps clamped into the source whatever the map holds.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                  // output pixels per thread of the gather: 12 bytes = three dwords
constexpr int kMaxSide = 1 << 21;        // (side - 1) * 1024 stays an int32

enum { SIMPLE_RADIAL = 2, RADIAL = 3, OPENCV = 4, OPENCV_FISHEYE = 5, FULL_OPENCV = 6, SIMPLE_RADIAL_FISHEYE = 8,
       RADIAL_FISHEYE = 9, THIN_PRISM_FISHEYE = 10 };

struct MapArgs {
  double fxs, fys, cxs, cys;             // the distorted camera
  double c[8];                           // its coefficients in COLMAP's order
  double fx, fy, cx, cy;                 // the undistorted camera
  int W, H, Wo, Ho;
};

// (u, v) -> (u_d, v_d).  Every line is the restatement's (tests/undistort_restated.py, atvsnet/undistort.py distort): same
// operands, same order, products and sums evaluated left to right.
template <int MODEL>
__device__ __forceinline__ void distort(const double* __restrict__ c, double u, double v, double* ud, double* vd) {
  const double r2 = u * u + v * v;
  if (MODEL == SIMPLE_RADIAL || MODEL == RADIAL) {
    const double r4 = r2 * r2;
    const double rad = MODEL == SIMPLE_RADIAL ? c[0] * r2 : c[0] * r2 + c[1] * r4;
    *ud = u + u * rad;
    *vd = v + v * rad;
  } else if (MODEL == OPENCV) {
    const double r4 = r2 * r2;
    const double rad = c[0] * r2 + c[1] * r4;
    const double p1 = c[2], p2 = c[3];
    *ud = u + u * rad + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u);
    *vd = v + v * rad + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v);
  } else if (MODEL == FULL_OPENCV) {
    const double r4 = r2 * r2, r6 = r4 * r2;
    const double p1 = c[2], p2 = c[3];
    const double rad = (1.0 + c[0] * r2 + c[1] * r4 + c[4] * r6) / (1.0 + c[5] * r2 + c[6] * r4 + c[7] * r6);
    *ud = u * rad + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u);
    *vd = v * rad + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v);
  } else {                               // the fisheye family
    const double r = sqrt(r2);
    const double theta = atan(r);
    const bool off_axis = r > 1e-8;
    const double uu = off_axis ? u * theta / r : u;
    const double vv = off_axis ? v * theta / r : v;
    const double t2 = uu * uu + vv * vv;
    const double t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
    if (MODEL == SIMPLE_RADIAL_FISHEYE || MODEL == RADIAL_FISHEYE) {
      const double rad = MODEL == SIMPLE_RADIAL_FISHEYE ? c[0] * t2 : c[0] * t2 + c[1] * t4;
      *ud = uu + uu * rad;
      *vd = vv + vv * rad;
    } else if (MODEL == OPENCV_FISHEYE) {
      const double rad = c[0] * t2 + c[1] * t4 + c[2] * t6 + c[3] * t8;
      *ud = uu + uu * rad;
      *vd = vv + vv * rad;
    } else {                             // THIN_PRISM_FISHEYE: k1, k2, p1, p2, k3, k4, sx1, sy1
      const double rad = c[0] * t2 + c[1] * t4 + c[4] * t6 + c[5] * t8;
      const double p1 = c[2], p2 = c[3];
      *ud = uu + uu * rad + 2.0 * p1 * uu * vv + p2 * (t2 + 2.0 * uu * uu) + c[6] * t2;
      *vd = vv + vv * rad + 2.0 * p2 * uu * vv + p1 * (t2 + 2.0 * vv * vv) + c[7] * t2;
    }
  }
}

template <int MODEL>
__global__ __launch_bounds__(kThreads) void undistort_map_kernel(const MapArgs a, int2* __restrict__ map) {
  const long n = (long)a.Wo * a.Ho;
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int Y = (int)(i / a.Wo), X = (int)(i - (long)Y * a.Wo);
  const double u = (((double)X + 0.5) - a.cx) / a.fx;
  const double v = (((double)Y + 0.5) - a.cy) / a.fy;
  double ud, vd;
  distort<MODEL>(a.c, u, v, &ud, &vd);
  const double sx = (a.fxs * ud + a.cxs) - 0.5;
  const double sy = (a.fys * vd + a.cys) - 0.5;
  const double qx = floor(sx * 1024.0 + 0.5);
  const double qy = floor(sy * 1024.0 + 0.5);
  // decided in float64: NaN fails every comparison, +-inf the range
  const bool valid = isfinite(sx) && isfinite(sy) && qx >= 0.0 && qx <= (double)((a.W - 1) * 1024) && qy >= 0.0 &&
                     qy <= (double)((a.H - 1) * 1024);
  map[i] = valid ? make_int2((int)qx, (int)qy) : make_int2(INT_MIN, 0);
}

__device__ __forceinline__ void sample(const uint8_t* __restrict__ src, int W, int H, int qx, int qy, unsigned* out) {
  // clamped: a map that does not belong to this source can give wrong pixels, never an out-of-bounds read
  const int x0 = min(max(qx >> 10, 0), W - 1), x1 = min(x0 + 1, W - 1);
  const int y0 = min(max(qy >> 10, 0), H - 1), y1 = min(y0 + 1, H - 1);
  const int fx = qx & 1023, fy = qy & 1023;
  const uint8_t* r0 = src + (long)y0 * W * 3;
  const uint8_t* r1 = src + (long)y1 * W * 3;
  const long o0 = (long)x0 * 3, o1 = (long)x1 * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int top = (int)r0[o0 + ch] * (1024 - fx) + (int)r0[o1 + ch] * fx;
    const int bot = (int)r1[o0 + ch] * (1024 - fx) + (int)r1[o1 + ch] * fx;
    out[ch] = (unsigned)((top * (1024 - fy) + bot * fy + (1 << 19)) >> 20);      // <= 255 * 2^20 + 2^19: an int32
  }
}

__global__ __launch_bounds__(kThreads) void undistort_remap_kernel(const uint8_t* __restrict__ src, int W, int H,
                                                                   const int* __restrict__ map, long n, uint8_t* __restrict__ dst) {
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  const long p0 = g * kPix;
  if (p0 >= n) return;
  if (p0 + kPix <= n) {
    const int4 m0 = reinterpret_cast<const int4*>(map)[g * 2], m1 = reinterpret_cast<const int4*>(map)[g * 2 + 1];
    const int q[2 * kPix] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    unsigned b[3 * kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0u;
      if (q[2 * k] != INT_MIN) sample(src, W, H, q[2 * k], q[2 * k + 1], b + 3 * k);
    }
    unsigned* o = reinterpret_cast<unsigned*>(dst) + g * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  } else {                               // the last thread: n mod 4 pixels, by bytes
    for (long p = p0; p < n; ++p) {
      unsigned b[3] = {0u, 0u, 0u};
      const int qx = map[2 * p], qy = map[2 * p + 1];
      if (qx != INT_MIN) sample(src, W, H, qx, qy, b);
      dst[3 * p] = (uint8_t)b[0];
      dst[3 * p + 1] = (uint8_t)b[1];
      dst[3 * p + 2] = (uint8_t)b[2];
    }
  }
}

bool sizes_ok(int W, int H, int Wo, int Ho) {
  return W >= 1 && H >= 1 && Wo >= 1 && Ho >= 1 && W <= kMaxSide && H <= kMaxSide && (long)W * H <= 0x7fffffffL &&
         (long)Wo * Ho <= 0x7fffffffL;
}

// the model's parameters -> fxs, fys, cxs, cys, c[8]; false for a model id this library does not undistort
bool split_params(int model_id, const double* p, MapArgs* a) {
  int n_coef, one_focal;
  switch (model_id) {
    case SIMPLE_RADIAL: case SIMPLE_RADIAL_FISHEYE: one_focal = 1; n_coef = 1; break;
    case RADIAL: case RADIAL_FISHEYE: one_focal = 1; n_coef = 2; break;
    case OPENCV: case OPENCV_FISHEYE: one_focal = 0; n_coef = 4; break;
    case FULL_OPENCV: case THIN_PRISM_FISHEYE: one_focal = 0; n_coef = 8; break;
    default: return false;
  }
  const double* c = p + (one_focal ? 3 : 4);
  a->fxs = p[0];
  a->fys = one_focal ? p[0] : p[1];
  a->cxs = one_focal ? p[1] : p[2];
  a->cys = one_focal ? p[2] : p[3];
  for (int k = 0; k < 8; ++k) a->c[k] = k < n_coef ? c[k] : 0.0;
  bool finite = std::isfinite(a->fxs) && std::isfinite(a->fys) && std::isfinite(a->cxs) && std::isfinite(a->cys);
  for (int k = 0; k < 8; ++k) finite = finite && std::isfinite(a->c[k]);
  return finite;
}

template <int MODEL>
void launch_map(const MapArgs& a, int* map, hipStream_t st) {
  hipLaunchKernelGGL(undistort_map_kernel<MODEL>, dim3((unsigned)cdiv((long)a.Wo * a.Ho, kThreads)), dim3(kThreads), 0, st, a,
                     reinterpret_cast<int2*>(map));
}

}  // namespace

extern "C" int atvs_undistort_map(int model_id, const double* params, int W, int H, const double* camera, int Wo, int Ho, int* map,
                                  atvs_stream_t stream) {
  if (!params || !camera || !map) return ATVS_ERR_NULL;
  MapArgs a;
  if (!sizes_ok(W, H, Wo, Ho) || !split_params(model_id, params, &a)) return ATVS_ERR_ARG;
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(camera[k])) return ATVS_ERR_ARG;
  if (camera[0] == 0.0 || camera[1] == 0.0 || (reinterpret_cast<uintptr_t>(map) & 15)) return ATVS_ERR_ARG;
  a.fx = camera[0], a.fy = camera[1], a.cx = camera[2], a.cy = camera[3];
  a.W = W, a.H = H, a.Wo = Wo, a.Ho = Ho;
  hipStream_t st = as_stream(stream);
  switch (model_id) {
    case SIMPLE_RADIAL: launch_map<SIMPLE_RADIAL>(a, map, st); break;
    case RADIAL: launch_map<RADIAL>(a, map, st); break;
    case OPENCV: launch_map<OPENCV>(a, map, st); break;
    case OPENCV_FISHEYE: launch_map<OPENCV_FISHEYE>(a, map, st); break;
    case FULL_OPENCV: launch_map<FULL_OPENCV>(a, map, st); break;
    case SIMPLE_RADIAL_FISHEYE: launch_map<SIMPLE_RADIAL_FISHEYE>(a, map, st); break;
    case RADIAL_FISHEYE: launch_map<RADIAL_FISHEYE>(a, map, st); break;
    default: launch_map<THIN_PRISM_FISHEYE>(a, map, st); break;       // split_params has refused every other id
  }
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_undistort_remap(const unsigned char* src, int W, int H, const int* map, int Wo, int Ho, unsigned char* dst,
                                    atvs_stream_t stream) {
  if (!src || !map || !dst) return ATVS_ERR_NULL;
  if (!sizes_ok(W, H, Wo, Ho) || (reinterpret_cast<uintptr_t>(map) & 15) || (reinterpret_cast<uintptr_t>(dst) & 3))
    return ATVS_ERR_ARG;
  const long n = (long)Wo * Ho;
  hipLaunchKernelGGL(undistort_remap_kernel, dim3((unsigned)cdiv(cdiv(n, kPix), kThreads)), dim3(kThreads), 0, as_stream(stream),
                     src, W, H, map, n, dst);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
