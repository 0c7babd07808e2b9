// The per-pixel body of the depth-map fusion (reference fusibile/fusibile.cu:138-277), shared by the per-camera kernel
// (fusion.hip, atvs_fusibile) and the whole-scene kernel (fusion_scene.hip, atvs_fusibile_scene): both call fuse_pixel, so a
// pixel's arithmetic is the same in the two by construction.  Its agreement loop is agreeing_views, which the support kernel
// (fusion_support.hip, atvs_fusion_support) calls without the colours.  All three sources are built with -ffp-contract=off.
//
// Arithmetic contract (oracle/fusibile.py, bit for bit): float32, left to right; the CUDA texture fetch
// tex2D<float4>(t, x + 0.5, y + 0.5) of an un-normalised linear texture is restated as the bilinear blend of texels floor(x),
// floor(x) + 1 (clamped to the image) with weights rounded to 8 fractional bits -- plain loads, no texture unit.
#pragma once
#include "common.h"

namespace {

struct Cam {      // 28 floats per camera: P[12] | M_inv[9] | C[3] | P_col34[3] | f
  const float* p;
  __device__ __forceinline__ float P(int i) const { return p[i]; }
  __device__ __forceinline__ float Mi(int i) const { return p[12 + i]; }
  __device__ __forceinline__ float C(int i) const { return p[21 + i]; }
  __device__ __forceinline__ float pc(int i) const { return p[24 + i]; }
  __device__ __forceinline__ float f() const { return p[27]; }
};

__device__ __forceinline__ float4 tex_fetch(const float4* __restrict__ tex, float x, float y, int rows, int cols) {
  const float xf = floorf(x), yf = floorf(y);
  const float ax = floorf((x - xf) * 256.0f + 0.5f) / 256.0f;
  const float ay = floorf((y - yf) * 256.0f + 0.5f) / 256.0f;
  const int xi = (int)xf, yi = (int)yf;
  const int x0 = min(max(xi, 0), cols - 1), x1 = min(max(xi + 1, 0), cols - 1);
  const int y0 = min(max(yi, 0), rows - 1), y1 = min(max(yi + 1, 0), rows - 1);
  const float4 a = tex[(size_t)y0 * cols + x0], b = tex[(size_t)y0 * cols + x1];
  const float4 c = tex[(size_t)y1 * cols + x0], d = tex[(size_t)y1 * cols + x1];
  const float bx = 1.0f - ax, by = 1.0f - ay;
  float4 top, bot, o;
  top.x = bx * a.x + ax * b.x; top.y = bx * a.y + ax * b.y; top.z = bx * a.z + ax * b.z; top.w = bx * a.w + ax * b.w;
  bot.x = bx * c.x + ax * d.x; bot.y = bx * c.y + ax * d.y; bot.z = bx * c.z + ax * d.z; bot.w = bx * c.w + ax * d.w;
  o.x = by * top.x + ay * bot.x; o.y = by * top.y + ay * bot.y; o.z = by * top.z + ay * bot.z; o.w = by * top.w + ay * bot.w;
  return o;
}

struct FusedPixel {
  float4 coord;     // the back-projected 3-D point (x, y, z, 0)
  float4 normal;    // normal averaged over the reference and the agreeing views (w = 0)
  float4 texture;   // colour (b, g, r) averaged likewise (w = 0)
  bool created;     // at least num_consistent other views agree
};

// The agreement loop of pixel (x, y) of reference camera `ref`, the one piece of code behind fuse_pixel and the support kernel
// (fusion_support.hip): back-project the pixel with its depth, project the 3-D point into every other view (ascending), sample that
// view's (normal, depth) map bilinearly, accept the view when it lands in the image, the relative disparity difference and the normal
// angle are under their thresholds.  -> the number of accepted views; X receives the 3-D point, cn the reference normal plus the
// accepted views' normals.  kImages: ct receives the reference colour plus the accepted views' colours; without it `img` is not
// read (it may be nullptr), ct is left alone, and the fetches are compiled out.
template <bool kImages>
__device__ __forceinline__ int agreeing_views(const float* __restrict__ cams, const float4* __restrict__ nd,
                                              const float4* __restrict__ img, int nviews, int ref, int rows, int cols, int x, int y,
                                              float disp_thresh, float normal_thresh, float4& X, float4& cn, float4& ct) {
  const size_t center = (size_t)y * cols + x, plane = (size_t)rows * cols;
  const Cam cr = {cams + (size_t)ref * 28};
  const float4 nrm = nd[(size_t)ref * plane + center];
  const float depth = nrm.w;
  // get3Dpoint_cu (:53-62)
  const float ptx = depth * (float)x - cr.pc(0), pty = depth * (float)y - cr.pc(1), ptz = depth - cr.pc(2);
  const float Xx = cr.Mi(0) * ptx + cr.Mi(1) * pty + cr.Mi(2) * ptz;
  const float Xy = cr.Mi(3) * ptx + cr.Mi(4) * pty + cr.Mi(5) * ptz;
  const float Xz = cr.Mi(6) * ptx + cr.Mi(7) * pty + cr.Mi(8) * ptz;
  cn = nrm;
  if constexpr (kImages) ct = img[(size_t)ref * plane + center];
  int count = 0;
  for (int i = 0; i < nviews; ++i) {
    if (i == ref) continue;
    const Cam c = {cams + (size_t)i * 28};
    // project_on_camera (:127-133)
    const float tx = c.P(0) * Xx + c.P(1) * Xy + c.P(2) * Xz + c.P(3);
    const float ty = c.P(4) * Xx + c.P(5) * Xy + c.P(6) * Xz + c.P(7);
    const float tz = c.P(8) * Xx + c.P(9) * Xy + c.P(10) * Xz + c.P(11);
    const float px = tx / tz, py = ty / tz, d = tz;
    if (!(px >= 0.f && px < (float)cols && py >= 0.f && py < (float)rows)) continue;
    const float4 other = tex_fetch(nd + (size_t)i * plane, px, py, rows, cols);
    const float dx = cr.C(0) - c.C(0), dy = cr.C(1) - c.C(1), dz = cr.C(2) - c.C(2);
    const float base = sqrtf(dx * dx + dy * dy + dz * dz);
    const float fb = cr.f() * base;
    const float d_disp = fb / d, o_disp = fb / other.w;
    if (!((fabsf(d_disp - o_disp) / d_disp) < disp_thresh)) continue;
    const float dot = other.x * nrm.x + other.y * nrm.y + other.z * nrm.z;
    float ang = acosf(dot);
    if (ang != ang) ang = 0.f;
    if (!(ang < normal_thresh)) continue;
    cn = make_float4(cn.x + other.x, cn.y + other.y, cn.z + other.z, 0.f);
    if constexpr (kImages) {
      const float4 t = tex_fetch(img + (size_t)i * plane, px, py, rows, cols);
      ct = make_float4(ct.x + t.x, ct.y + t.y, ct.z + t.z, 0.f);
    }
    ++count;
  }
  X = make_float4(Xx, Xy, Xz, 0.f);
  return count;
}

// Pixel (x, y) of reference camera `ref`: the agreement loop above with the colours, then normals and colours averaged over the
// reference and the accepted views.
__device__ __forceinline__ FusedPixel fuse_pixel(const float* __restrict__ cams, const float4* __restrict__ nd,
                                                 const float4* __restrict__ img, int nviews, int ref, int rows, int cols, int x,
                                                 int y, float disp_thresh, float normal_thresh, int num_consistent) {
  float4 X, cn, ct;
  const int count = agreeing_views<true>(cams, nd, img, nviews, ref, rows, cols, x, y, disp_thresh, normal_thresh, X, cn, ct);
  const float k = (float)count + 1.0f;
  FusedPixel o;
  o.coord = X;
  o.normal = make_float4(cn.x / k, cn.y / k, cn.z / k, 0.f);
  o.texture = make_float4(ct.x / k, ct.y / k, ct.z / k, 0.f);
  o.created = count >= num_consistent;
  return o;
}

}  // namespace
