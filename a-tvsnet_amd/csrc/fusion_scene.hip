// Scene-resident depth-map fusion (gfx950): the maps of a whole scene staged on the device and fused in one pass.
//
// atvs_fusion_stage_f32 turns one finished depth map into its slot of the scene slab: per pixel exactly what the file pipeline
// computes on the host (eval_pointcloud._write_map's inverse-depth step, depth_fusion.probability_filter, fake_colmap_normal).
//
// atvs_fusibile_scene fuses every reference camera of the slab and compacts the kept points in the order of
// depth_fusion.fuse_views (camera-major, row-major within a camera), in three launches:
//   count    one workgroup per (camera, run of 256 row-major pixels): fuse_pixel (fusion_pixel.h, the per-camera kernel's body),
//            the host filter (created and three non-zero coordinates), the kept points compacted IN ORDER into the
//            workgroup's own 256-entry region of the scratch, their number into counts[workgroup];
//   scan     one workgroup: exclusive scan of the counts (workgroups are numbered camera-major, so the scan is the output order),
//            and the total;
//   scatter  one workgroup per count: its region to points / colours at its offset.
// No workgroup waits on another, no atomics; the cameras are wave-uniform (one reference per workgroup).
//
// atvs_fusibile_scene_normals is the same three launches with kNormals = true: the count pass also keeps fuse_pixel's averaged
// normal of every kept point in a second region of the scratch, the scatter pass writes it beside the point.
#include "fusion_grid.h"
#include "fusion_pixel.h"

namespace {

constexpr int kScanThreads = 1024;

struct ScratchLayout {               // byte offsets into the caller's scratch
  size_t counts, offsets, slab, nslab, bytes;
};

__host__ __device__ inline ScratchLayout scratch_layout(long blocks, bool normals) {
  ScratchLayout s;
  s.counts = 0;
  s.offsets = ((size_t)blocks * 4 + 255) & ~(size_t)255;
  s.slab = s.offsets + (((size_t)blocks * 4 + 255) & ~(size_t)255);
  s.nslab = s.slab + (size_t)blocks * kRun * sizeof(float4);
  s.bytes = s.nslab + (normals ? (size_t)blocks * kRun * sizeof(float4) : 0);
  return s;
}

__global__ __launch_bounds__(256) void fusion_stage_kernel(const float* __restrict__ depth, const float* __restrict__ prob,
                                                           const unsigned char* __restrict__ bgr, int n, int inverse_depth,
                                                           float prob_thresh, float4* __restrict__ nd_out,
                                                           float4* __restrict__ img_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float d = depth[i];
  if (inverse_depth) {                                  // m[m <= 0] = inf; depth = 1 / m  (float32, correctly rounded)
    if (d <= 0.f) d = __builtin_inff();
    d = __fdiv_rn(1.0f, d);
  }
  if (prob[i] < prob_thresh) d = 0.f;                   // depth[prob < threshold] = 0
  // fake_colmap_normal: float32(1) / float32(1.732050808) where depth > 0, else +0
  const float nv = (d > 0.f) ? __fdiv_rn(1.0f, (float)1.732050808) : 0.f;
  nd_out[i] = make_float4(nv, nv, nv, d);
  const unsigned char* p = bgr + (size_t)i * 3;
  img_out[i] = make_float4((float)p[0], (float)p[1], (float)p[2], 0.f);
}

template <bool kNormals>
__global__ __launch_bounds__(kRun) void fusion_count_kernel(const float* __restrict__ cams, const float4* __restrict__ nd,
                                                            const float4* __restrict__ img, int nviews, int rows, int cols,
                                                            int runs_per_cam, float disp_thresh, float normal_thresh,
                                                            int num_consistent, int* __restrict__ counts,
                                                            float4* __restrict__ slab, float4* __restrict__ nslab) {
  __shared__ int wave_kept[kRun / 64];
  const int b = blockIdx.x;
  const int ref = b / runs_per_cam;                    // uniform over the workgroup
  const int p = (b - ref * runs_per_cam) * kRun + (int)threadIdx.x;
  bool keep = false;
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f), nout = out;
  if (p < rows * cols) {
    const int y = p / cols, x = p - y * cols;
    const FusedPixel o = fuse_pixel(cams, nd, img, nviews, ref, rows, cols, x, y, disp_thresh, normal_thresh, num_consistent);
    keep = o.created && o.coord.x != 0.f && o.coord.y != 0.f && o.coord.z != 0.f;
    // (char)(int) of channels 2, 1, 0 of the averaged texture (fusibile/displayUtils.h:109-111), packed r | g << 8 | b << 16
    const unsigned r = (unsigned char)(int)o.texture.z, g = (unsigned char)(int)o.texture.y, bl = (unsigned char)(int)o.texture.x;
    out = make_float4(o.coord.x, o.coord.y, o.coord.z, __uint_as_float(r | (g << 8) | (bl << 16)));
    nout = o.normal;
  }
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_kept[wave] = __popcll(m);
  __syncthreads();
  int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < kRun / 64; ++w) {
    if (w < wave) before += wave_kept[w];
    total += wave_kept[w];
  }
  if (keep) slab[(size_t)b * kRun + before] = out;
  if (kNormals && keep) nslab[(size_t)b * kRun + before] = nout;
  if (threadIdx.x == 0) counts[b] = total;
}

__global__ __launch_bounds__(kScanThreads) void fusion_scan_kernel(const int* __restrict__ counts, int blocks,
                                                                   int* __restrict__ offsets, int* __restrict__ total) {
  __shared__ int buf[kScanThreads];
  int carry = 0;
  for (int base = 0; base < blocks; base += kScanThreads) {
    const int i = base + (int)threadIdx.x;
    const int v = i < blocks ? counts[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int step = 1; step < kScanThreads; step <<= 1) {     // inclusive Hillis-Steele scan of this chunk
      const int add = (int)threadIdx.x >= step ? buf[threadIdx.x - step] : 0;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < blocks) offsets[i] = carry + buf[threadIdx.x] - v;
    carry += buf[kScanThreads - 1];
    __syncthreads();                                          // buf is rewritten by the next chunk
  }
  if (threadIdx.x == 0) total[0] = carry;
}

template <bool kNormals>
__global__ __launch_bounds__(kRun) void fusion_scatter_kernel(const int* __restrict__ counts, const int* __restrict__ offsets,
                                                              const float4* __restrict__ slab, const float4* __restrict__ nslab,
                                                              long capacity, float* __restrict__ points,
                                                              unsigned char* __restrict__ colors, float* __restrict__ normals) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= counts[b]) return;
  const long dst = (long)offsets[b] + t;
  if (dst >= capacity) return;
  const float4 v = slab[(size_t)b * kRun + t];
  const unsigned rgb = __float_as_uint(v.w);
  points[dst * 3 + 0] = v.x;
  points[dst * 3 + 1] = v.y;
  points[dst * 3 + 2] = v.z;
  colors[dst * 3 + 0] = (unsigned char)(rgb & 0xff);
  colors[dst * 3 + 1] = (unsigned char)((rgb >> 8) & 0xff);
  colors[dst * 3 + 2] = (unsigned char)((rgb >> 16) & 0xff);
  if (kNormals) {
    const float4 n = nslab[(size_t)b * kRun + t];
    normals[dst * 3 + 0] = n.x;
    normals[dst * 3 + 1] = n.y;
    normals[dst * 3 + 2] = n.z;
  }
}

int scene_scratch_size(int nviews, int rows, int cols, bool normals, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  int runs = 0;
  long blocks = 0;
  if (!scene_grid(nviews, rows, cols, &runs, &blocks)) return ATVS_ERR_SHAPE;
  *bytes = (long)scratch_layout(blocks, normals).bytes;
  return ATVS_OK;
}

// count, scan, scatter on `stream`; kNormals: `normals` (capacity, 3) receives fuse_pixel's normal.xyz of every kept point
template <bool kNormals>
int fuse_scene(const float* cams, const float* normals_depths, const float* images, int nviews, int rows, int cols,
               float disp_thresh, float normal_thresh, int num_consistent, void* scratch, long scratch_bytes, float* points,
               unsigned char* colors, float* normals, long capacity, int* n_points, atvs_stream_t stream) {
  if (!cams || !normals_depths || !images || !scratch || !points || !colors || !n_points || (kNormals && !normals))
    return ATVS_ERR_NULL;
  int runs = 0;
  long blocks = 0;
  if (!scene_grid(nviews, rows, cols, &runs, &blocks)) return ATVS_ERR_SHAPE;
  const ScratchLayout L = scratch_layout(blocks, kNormals);
  // every pixel may become a point: the outputs must hold N * rows * cols of them
  if (scratch_bytes < (long)L.bytes || capacity < (long)nviews * rows * cols) return ATVS_ERR_SHAPE;
  char* s = static_cast<char*>(scratch);
  int* counts = reinterpret_cast<int*>(s + L.counts);
  int* offsets = reinterpret_cast<int*>(s + L.offsets);
  float4* slab = reinterpret_cast<float4*>(s + L.slab);
  float4* nslab = kNormals ? reinterpret_cast<float4*>(s + L.nslab) : nullptr;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(fusion_count_kernel<kNormals>, dim3((unsigned)blocks), dim3(kRun), 0, st, cams,
                     reinterpret_cast<const float4*>(normals_depths), reinterpret_cast<const float4*>(images), nviews, rows, cols,
                     runs, disp_thresh, normal_thresh, num_consistent, counts, slab, nslab);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fusion_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, counts, (int)blocks, offsets, n_points);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fusion_scatter_kernel<kNormals>, dim3((unsigned)blocks), dim3(kRun), 0, st, counts, offsets, slab, nslab,
                     capacity, points, colors, normals);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

}  // namespace

extern "C" int atvs_fusion_stage_f32(const float* depth, const float* prob, const unsigned char* bgr, int rows, int cols,
                                     int inverse_depth, float prob_thresh, float* nd_out, float* img_out, atvs_stream_t stream) {
  if (!depth || !prob || !bgr || !nd_out || !img_out) return ATVS_ERR_NULL;
  if (rows <= 0 || cols <= 0 || (long long)rows * cols > 0x7fffffffLL - 256) return ATVS_ERR_SHAPE;
  if (inverse_depth != 0 && inverse_depth != 1) return ATVS_ERR_ARG;
  const int n = rows * cols;
  hipLaunchKernelGGL(fusion_stage_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), depth, prob, bgr, n, inverse_depth,
                     prob_thresh, reinterpret_cast<float4*>(nd_out), reinterpret_cast<float4*>(img_out));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_fusibile_scene_scratch_size(int nviews, int rows, int cols, long* bytes) {
  return scene_scratch_size(nviews, rows, cols, false, bytes);
}

extern "C" int atvs_fusibile_scene_normals_scratch_size(int nviews, int rows, int cols, long* bytes) {
  return scene_scratch_size(nviews, rows, cols, true, bytes);
}

extern "C" int atvs_fusibile_scene(const float* cams, const float* normals_depths, const float* images, int nviews, int rows,
                                   int cols, float disp_thresh, float normal_thresh, int num_consistent, void* scratch,
                                   long scratch_bytes, float* points, unsigned char* colors, long capacity, int* n_points,
                                   atvs_stream_t stream) {
  return fuse_scene<false>(cams, normals_depths, images, nviews, rows, cols, disp_thresh, normal_thresh, num_consistent, scratch,
                           scratch_bytes, points, colors, nullptr, capacity, n_points, stream);
}

extern "C" int atvs_fusibile_scene_normals(const float* cams, const float* normals_depths, const float* images, int nviews,
                                           int rows, int cols, float disp_thresh, float normal_thresh, int num_consistent,
                                           void* scratch, long scratch_bytes, float* points, unsigned char* colors, float* normals,
                                           long capacity, int* n_points, atvs_stream_t stream) {
  return fuse_scene<true>(cams, normals_depths, images, nviews, rows, cols, disp_thresh, normal_thresh, num_consistent, scratch,
                          scratch_bytes, points, colors, normals, capacity, n_points, stream);
}
