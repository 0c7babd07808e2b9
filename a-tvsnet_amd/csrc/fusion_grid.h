// The workgroup grid of the whole-scene fusion kernels (fusion_scene.hip, depth_normals.hip): a workgroup owns a run of kRun
// row-major pixels of ONE camera, so the camera's 28 floats are wave-uniform; workgroups are numbered camera-major.
#pragma once

namespace {

constexpr int kRun = 256;            // pixels per workgroup (4 waves)

// runs of kRun pixels per camera and workgroups of one pass over the slab; false when the index types cannot hold the scene
inline bool scene_grid(int nviews, int rows, int cols, int* runs_per_cam, long* blocks) {
  if (nviews <= 0 || rows <= 0 || cols <= 0) return false;
  const long long plane = (long long)rows * cols;
  const long long runs = (plane + kRun - 1) / kRun;
  // every pixel index of the slab (N * rows * cols), every slot of the scratch regions (blocks * kRun) and the point count: int
  if (plane * nviews > 0x7fffffffLL || runs * kRun * nviews > 0x7fffffffLL) return false;
  *runs_per_cam = (int)runs;
  *blocks = (long)(runs * nviews);
  return true;
}

}  // namespace
