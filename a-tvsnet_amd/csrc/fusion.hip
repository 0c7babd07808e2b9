// Depth-map fusion by cross-view consistency voting (gfx950): the `fusibile` kernel of the reference's point-cloud
// stage, /root/reference/fusibile/fusibile.cu:138-277 (called per reference camera from :422-427; cameras from
// cameraGeometryUtils.h:194-499, textures from main.cpp:459-498).
//
// One thread per pixel of the reference camera: back-project the pixel with its depth, project the 3-D point into
// every other view, sample that view's (normal, depth) map and colour bilinearly, accept the view when the relative
// disparity difference and the normal angle are under their thresholds, average normals and colours over the
// accepted views, and create the point when enough views agree (fuse_pixel, fusion_pixel.h; the whole-scene form of
// this launch is fusion_scene.hip).  HBM / L2-bound gathers (N - 1 bilinear float4 fetches x 2 per pixel); no matrix work.
//
// Arithmetic contract: fusion_pixel.h (oracle/fusibile.py bit for bit; built with -ffp-contract=off).
#include "fusion_pixel.h"

namespace {

__global__ __launch_bounds__(256) void fusibile_kernel(const float* __restrict__ cams, const float4* __restrict__ nd,
                                                       const float4* __restrict__ img, int nviews, int ref, int rows,
                                                       int cols, float disp_thresh, float normal_thresh, int num_consistent,
                                                       float4* __restrict__ coord, float4* __restrict__ normal_out,
                                                       float4* __restrict__ tex_out, float* __restrict__ created) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= cols || y >= rows) return;
  const size_t center = (size_t)y * cols + x;
  const FusedPixel o = fuse_pixel(cams, nd, img, nviews, ref, rows, cols, x, y, disp_thresh, normal_thresh, num_consistent);
  coord[center] = o.coord;
  normal_out[center] = o.normal;
  tex_out[center] = o.texture;
  created[center] = o.created ? 1.f : 0.f;
}

}  // namespace


// cams (nviews, 28) floats per camera: P[12] | M_inv[9] | C[3] | P_col34[3] | f_ref-candidate (K[0,0]); normals_depths and
// images (nviews, rows, cols, 4) float: (nx, ny, nz, depth) and (b, g, r, unused).  Outputs for reference camera `ref`,
// each (rows, cols, 4) resp. (rows, cols): the 3-D point of every pixel, the averaged normal and colour, and 1 / 0 for
// "at least num_consistent other views agree" (the reference stores the point only then, fusibile.cu:252-262).
extern "C" int atvs_fusibile(const float* cams, const float* normals_depths, const float* images, int nviews, int ref,
                             int rows, int cols, float disp_thresh, float normal_thresh, int num_consistent, float* coord,
                             float* normal, float* texture, float* created, atvs_stream_t stream) {
  if (!cams || !normals_depths || !images || !coord || !normal || !texture || !created) return ATVS_ERR_NULL;
  if (nviews <= 0 || ref < 0 || ref >= nviews || rows <= 0 || cols <= 0) return ATVS_ERR_SHAPE;
  dim3 grid(cdiv(cols, 32), cdiv(rows, 8)), block(256);
  hipLaunchKernelGGL(fusibile_kernel, grid, block, 0, as_stream(stream), cams, reinterpret_cast<const float4*>(normals_depths),
                     reinterpret_cast<const float4*>(images), nviews, ref, rows, cols, disp_thresh, normal_thresh,
                     num_consistent, reinterpret_cast<float4*>(coord), reinterpret_cast<float4*>(normal),
                     reinterpret_cast<float4*>(texture), created);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
