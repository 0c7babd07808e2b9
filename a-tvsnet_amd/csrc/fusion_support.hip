// The fusion's agreement count per pixel (gfx950): for every pixel of every camera of a scene's slab, how many OTHER views agree on
// its depth -- fuse_pixel's `count`, from the very loop the fusion runs (fusion_pixel.h, agreeing_views), without the colour fetches
// and without the compaction.  From the count: the depth plane masked as the fusion masks its points (count >= num_consistent), and
// a per-pixel view weight (1 + count) / (1 + num_consistent) for the TSDF integration (tsdf.hip, atvs_tsdf_integrate_weighted).
//
// One launch shaped as fusion_scene.hip's count pass: one workgroup per (camera, run of 256 row-major pixels), so the reference
// camera's 28 floats are wave-uniform.  A lane owns one pixel and writes its own words of the outputs that were asked for: no
// atomics, no scratch, no workgroup waits on another, the same inputs give the same bits.
#include "fusion_grid.h"
#include "fusion_pixel.h"

namespace {

__global__ __launch_bounds__(kRun) void fusion_support_kernel(const float* __restrict__ cams, const float4* __restrict__ nd, int nviews,
                                                              int rows, int cols, int runs_per_cam, float disp_thresh,
                                                              float normal_thresh, int num_consistent, float denominator,
                                                              int* __restrict__ count_out, float* __restrict__ depth_out,
                                                              float* __restrict__ weight_out) {
  const int b = blockIdx.x;
  const int ref = b / runs_per_cam;                    // uniform over the workgroup
  const int p = (b - ref * runs_per_cam) * kRun + (int)threadIdx.x;
  if (p >= rows * cols) return;                        // no barrier follows
  const int y = p / cols, x = p - y * cols;
  float4 X, cn, ct;
  const int count = agreeing_views<false>(cams, nd, nullptr, nviews, ref, rows, cols, x, y, disp_thresh, normal_thresh, X, cn, ct);
  const size_t o = (size_t)ref * ((size_t)rows * cols) + (size_t)p;
  if (count_out != nullptr) count_out[o] = count;
  if (depth_out != nullptr) depth_out[o] = count >= num_consistent ? nd[o].w : 0.f;
  if (weight_out != nullptr) weight_out[o] = __fdiv_rn((float)(1 + count), denominator);
}

}  // namespace

extern "C" int atvs_fusion_support(const float* cams, const float* normals_depths, int nviews, int rows, int cols, float disp_thresh,
                                   float normal_thresh, int num_consistent, int* count, float* depth_out, float* weight_out,
                                   atvs_stream_t stream) {
  if (!cams || !normals_depths || (!count && !depth_out && !weight_out)) return ATVS_ERR_NULL;
  int runs = 0;
  long blocks = 0;
  if (!scene_grid(nviews, rows, cols, &runs, &blocks)) return ATVS_ERR_SHAPE;
  if (num_consistent < 0) return ATVS_ERR_ARG;
  hipLaunchKernelGGL(fusion_support_kernel, dim3((unsigned)blocks), dim3(kRun), 0, as_stream(stream), cams,
                     reinterpret_cast<const float4*>(normals_depths), nviews, rows, cols, runs, disp_thresh, normal_thresh, num_consistent,
                     (float)(1LL + (long long)num_consistent), count, depth_out, weight_out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
